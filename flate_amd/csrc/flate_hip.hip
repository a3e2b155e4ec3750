// flate_hip.hip -- host side of libflate_hip.so: the C ABI of include/flate_hip.h.
// Owns the device workspace, builds the chunk / block tables, launches the
// kernels on the caller's HIP stream.  There is no CPU execution path: without a
// usable gfx950 device every entry point fails.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <chrono>
#include <deque>
#include <vector>
#include <thread>

#include "../../include/flate_hip.h"
#include "kernels_block.h"
#include "kernels_common.h"
#include "dict_compress_plan.h"
#include "index_parts_plan.h"
#include "index_plan.h"
#include "index_scan_plan.h"
#include "inflate_plan.h"
#include "join_plan.h"
#include "kernels_deflater.h"
#include "kernels_dict.h"
#include "kernels_index.h"
#include "kernels_index_parts.h"
#include "kernels_index_scan.h"
#include "kernels_inflate.h"
#include "kernels_inflate_par.h"
#include "kernels_inflate_size.h"
#include "kernels_join.h"
#include "kernels_lz.h"
#include "kernels_members.h"
#include "kernels_parse.h"
#include "kernels_walk.h"
#include "kernels_stream.h"
#include "member_plan.h"
#include "pass_plan.h"
#include "size_plan.h"
#include "span_plan.h"
#include "stream_plan.h"
#include "stream_tables.h"

namespace {

enum KernelId {
    K_MEMSET = 0,
    K_BYTE_HIST,
    K_CHECKSUM,
    K_LZ_SORT,
    K_LZ_MATCH,
    K_LZ_CHAIN,
    K_LZ_PARSE,
    K_LZ_LINKS,
    K_LZ_WALK,
    K_LZ_EMIT,
    K_ST_PARSE,
    K_ST_EMIT,
    K_PLAN,
    K_OFFSETS,
    K_ENCODE,
    K_INFLATE,
    K_INFLATE_PAR,
    K_SPAN_SCAN,
    K_INFLATE_SPAN,
    K_INFLATE_SIZE,
    K_INFLATE_SIZE_SPAN,
    K_MEMBER_SCAN,
    K_MEMBER_CHAIN,
    K_MEMBER_WALK,
    K_MEMBER_PACK,
    K_MEMBER_FOLD,
    K_GATHER,
    K_INFLATER,
    K_DEFLATER,
    K_INFLATE_DICT,
    K_DICT_STAGE,
    K_JOIN_OPEN,
    K_JOIN_SCAN,
    K_JOIN_PACK,
    K_INDEX_WALK,
    K_INDEX_WINDOWS,
    K_INFLATE_RANGE,
    K_RANGE_PACK,
    K_JOIN_POINTS,
    K_INFLATE_PART,
    K_RANGE_SETTLE,
    K_INDEX_SCAN,
    K_COUNT
};
const char* const kKernelNames[K_COUNT] = {"memset_out", "k_byte_hist", "k_checksum", "k_lz_sort", "k_lz_match",
                                           "k_lz_chain", "k_lz_parse", "k_lz_links", "k_lz_walk", "k_lz_emit",
                                           "k_st_parse", "k_st_emit", "k_plan",
                                           "k_offsets",  "k_encode",    "k_inflate",  "k_inflate_par", "k_span_scan", "k_inflate_span",
                                           "k_inflate_size", "k_inflate_size_span",
                                           "k_member_scan", "k_member_chain", "k_member_walk", "k_member_pack", "k_member_fold",
                                           "k_gather", "k_inflater", "k_deflater", "k_inflate_dict", "k_dict_stage",
                                           "k_join_open", "k_join_scan", "k_join_pack",
                                           "k_index_walk", "k_index_windows", "k_inflate_range", "k_range_pack",
                                           "k_join_points", "k_inflate_part", "k_range_settle", "k_index_scan"};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
struct PinBuf {  // pinned host memory the handle keeps (pin_grow)
    void* p = nullptr;
    size_t cap = 0;
};

// The pieces of a flate_hip_compress_joined call, as compress_impl is handed them: a batch of raw chunks whose offsets are
// on the host already (input offsets of the pieces, their scratch slots), and what k_join_open needs behind every pass.
struct JoinCall {
    std::vector<uint64_t> hin, hout;
    int container = 0;  // of the joined streams (the pieces are raw)
    const uint32_t* d_piece_stream = nullptr;
    const fl_join_stream* d_streams = nullptr;
    uint32_t* d_piece_cks = nullptr;
};

// What flate_hip_compress_joined_indexed asks of the joined call beyond its outputs (index_parts_plan.h): the pieces that
// are points, and where k_join_scan put them.
struct JoinIndex {
    uint64_t spacing = 0;
    std::vector<fl_join_stream> streams;  // of the call (offsets less the staging shifts)
    std::vector<uint64_t> n_which;        // per stream: how many of its pieces are points
    std::vector<uint64_t> which;          // those pieces stream by stream, by their number within the stream
    std::vector<uint64_t> place;          // piece_dst of each, once the stream has been waited for
};

}  // namespace

// Offsets and per-pass tables of a compress batch whose layout does not change from call to call
// (flate_hip_plan_compress): with them a call only enqueues kernels.
struct flate_hip_plan {
    std::vector<uint64_t> hin, hout;
    uint32_t n_chunks = 0;
    int container = 0, mode = 0;
    struct Pass {
        uint32_t nc = 0, nb = 0;
        void* chunks = nullptr;     // fl_chunk[nc]
        void* blk_chunk = nullptr;  // uint32_t[nb]
    };
    std::vector<Pass> passes;
    bool ready = false;
};

// The tuning knobs of the environment, read ONCE when the handle is made -- no getenv on any call path
// (flate_hip_debug_reload_env reads them again: the test suite's seam).
struct fl_knobs {
    size_t max_pass_chunks = 32768;       // FLATE_HIP_MAX_PASS_CHUNKS
    // host-buffer calls whose buffers are pinned run in sub-batches of this many chunks, so that the H2D copy of
    // sub-batch k + 1 and the D2H copy of k - 1 overlap the kernels of k
    size_t host_pass_chunks = 1024;       // FLATE_HIP_HOST_PASS_CHUNKS
    uint64_t stream_pass_bytes = 4096ull << 20;  // FLATE_HIP_MAX_STREAM_PASS_MIB: whole-stream passes, uncompressed bytes per pass (about 30 bytes of scratch per input byte)
    uint64_t span_min_bytes = 0;          // FLATE_HIP_INFLATE_SPANS (0 = never); set to the default below
    bool span_debug = false;              // FLATE_HIP_SPAN_DEBUG
    int span_twin = -1;                   // FLATE_HIP_SPAN_TWIN: -1 unset, 0 never, 2..950 where to cut
    bool memset_inline = false;           // FLATE_HIP_MEMSET_INLINE: the output slots are cleared in the caller's stream (round 4's way; tuning)
    bool span_two_runs = false;           // FLATE_HIP_SPAN_TWO_RUNS: round 4's two decodes per span instead of one in symbols (tests, tuning)
    bool no_pin_mirror = false;           // FLATE_HIP_NO_PIN_MIRROR
    bool no_ramp = false;                 // FLATE_HIP_NO_RAMP
    uint32_t stream_group = 0;            // FLATE_HIP_STREAM_GROUP: windows per group of the whole-stream path (0: by the number of streams; tuning / tests)
    int stream_windows = -1;              // FLATE_HIP_STREAM_WINDOWS: -1 unset (by estimate), 0 never, 1 whenever possible (kernels_parse.h, k_lz_parse<true>)
    bool simple_ck_inline = false;        // FLATE_HIP_SIMPLE_CK_INLINE: the simple modes' checksum on the compute stream (round 4's way)
    bool one_stream = false;              // FLATE_HIP_ONE_COMPUTE_STREAM: the pinned path's sub-batches one after the other on the caller's stream (round 5's way; tuning)
    int rect = -1;                        // FLATE_HIP_RECT: 1 = half of every slot goes home by the DMA engine's rectangle copy (off by default: see there)
    int64_t inflate_par = -1;             // FLATE_HIP_INFLATE_PAR: -1 unset, 0 never, else the minimum stream size
    int64_t inflate_ring = -1;            // FLATE_HIP_INFLATE_RING: -1 unset
    bool member_scan = true;              // FLATE_HIP_MEMBER_SCAN: 0 = gzip members are walked, not searched for (flate_hip_decompress_members)
    uint32_t member_candidates = FL_MEM_CAND_DEFAULT;  // FLATE_HIP_MEMBER_CANDIDATES: a call with more candidates than this walks
    uint64_t index_pass_bytes = FL_IDX_PASS_BYTES;     // FLATE_HIP_INDEX_PASS_BYTES: scratch of one pass of flate_hip_decompress_ranges
};

struct flate_hip_ctx {
    int device = 0;
    fl_knobs knobs;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool sync = true;
    uint32_t flags = 0;  // flate_hip_set_flags
    std::string last_error;
    fl_crc_consts crc{};
    // device workspace (grown on demand, reused across calls)
    DevBuf chunks, blk_chunk, plans, hist, cks, S, NC, rec, desc, marks, tokens, ntok, cflag, links, shard_sz;
    DevBuf wexit;  // per window and sub-pass: where the path left it; per group: its exit, its entry; a flag (kernels_parse.h, fix launch)
    DevBuf wchunks, swins;  // whole-stream passes on k_lz_parse<true>: the streams' windows as chunks, a table entry per stream
    PinBuf pin_in, pin_out;  // pinned mirrors of pageable host buffers (run_on_mirrors)
    PinBuf pin_len;          // out_len of a sub-batch on its way home (Mirror::copy_out reads it before the call ends)
    PinBuf pin_tab;          // the pinned path's per-pass tables on their way to the device (a copy from PAGEABLE memory is staged by the runtime)
    uint32_t n_cu = 0;  // of the device (spans)
    DevBuf sp_points, sp_found, sp_spans, sp_res, sp_cand, sp_candoff, sp_tails, sp_tails_b, sp_chain, sp_chainoff,
        sp_pool, sp_pooltab, sp_poolctl, sp_items, sp_part, sp_footoff, sp_foot, sp_fin, sp_chainpos, sp_rs;  // inflate of long streams by spans
    DevBuf tiles, segs, pieces, fpts, zones, nsorted, jmp, exitmap, entry, segtok, tokbase, bound;  // whole-stream passes
    DevBuf sgroups, sgroup0, gmap, gentry, sblocks;
    DevBuf st_in, st_out, st_inoff, st_outlen, st_status, st_consumed, st_pack, st_packoff, st_slot;
    // host-buffer calls with pinned memory: copy streams beside the compute stream, events between them
    hipStream_t s_in = nullptr, s_out = nullptr;
    std::vector<hipEvent_t> xfer_events;
    // the container's checksum runs on a stream of its own beside the tokenizer (it reads the input and nothing else;
    // k_offsets waits for it)
    hipStream_t s_ck = nullptr;
    hipEvent_t ck_ev0 = nullptr, ck_ev1 = nullptr;
    hipStream_t s_c2 = nullptr;  // pinned path, round 6: every other sub-batch's kernels run here, beside the caller's stream (compress_impl)
    hipEvent_t c2_ev0 = nullptr, c2_ev1 = nullptr;
    hipStream_t s_ms = nullptr;  // the output slots are cleared beside the tokenizer / the histograms (round 5)
    hipEvent_t ms_ev0 = nullptr, ms_ev1 = nullptr;
    bool ms_pending = false;
    bool ck_pending = false;
    uint64_t dfl_bytes = 0;  // device memory the handle's deflaters hold (flate_hip_debug_device_bytes)
    uint64_t ws_bytes = 0;   // device memory ensure() holds for the handle (flate_hip_debug_workspace_bytes)
    // last flate_hip_decompress_batch call, for flate_hip_debug_inflate_paths: streams the span path took / finished,
    // streams k_inflate_par was launched for, and (counted on the device by k_inflate) those it handed on
    uint64_t dbg_span_taken = 0, dbg_span_done = 0, dbg_par_taken = 0;
    DevBuf dbg_par_handed;
    // flate_hip_decompress_batch_dict: the table of the call's dictionaries, and for host callers their bytes and dict_of
    DevBuf dc_tab, dc_bytes, dc_of;
    // flate_hip_compress_batch_dict, per pass of staged streams: history and record of every stream side by side, the staging
    // kernel's table, the chunk table of the records alone (the checksum's) -- dict_compress_plan.h
    DevBuf dcc_stage, dcc_jobs, dcc_chunks;
    // flate_hip_compress_joined: the pieces' scratch slots, the streams' table, and per piece its stream, its slot, its
    // length, status and checksum part, its place in its stream's slot; per stream the checksum -- join_plan.h.
    // `join`: such a call is running and its pieces are in compress_impl (enqueue_pass appends k_join_open to every pass)
    DevBuf jn_scratch, jn_streams, jn_pstream, jn_slot, jn_len, jn_status, jn_cks, jn_dst, jn_scks;
    DevBuf jn_which, jn_place;  // flate_hip_compress_joined_indexed: the point pieces and their places
    const JoinCall* join = nullptr;
    // flate_hip_decompressed_sizes: the span table and the span records of its long streams, and for
    // flate_hip_debug_size_paths the streams of the last call whose size came from a closed chain / from one wave
    DevBuf sz_spans, sz_recs;
    uint64_t dbg_size_chain = 0, dbg_size_whole = 0;
    // flate_hip_decompress_members: tile counts and their scan, the candidates with their chunks and probe results, the
    // successor and chain tables, the streams' member tables (as written and back to back), the members' decode results;
    // for flate_hip_debug_member_paths the last call's streams by path and its candidates that were on no chain
    DevBuf mb_tiles, mb_tileoff, mb_cand, mb_chunks, mb_psize, mb_pstatus, mb_pcons, mb_succ, mb_chain, mb_taboff, mb_tabn, mb_non,
        mb_tabstart, mb_tabsize, mb_denseoff, mb_dstart, mb_dsize, mb_outlen, mb_status, mb_cons, mb_nmem;
    uint64_t dbg_member[3] = {0, 0, 0};
    // flate_hip_index_build: the walk jobs, their records, the points as the walkers wrote them, the window copies' table;
    // flate_hip_decompress_ranges: the range jobs, the pack kernel's table, the scratch of a pass (index_plan.h); for
    // flate_hip_debug_index_passes the passes of the last ranges call
    DevBuf ix_jobs, ix_recs, ix_ptbit, ix_ptpos, ix_wtab, ix_rjobs, ix_rtab, ix_scratch;
    uint64_t dbg_index_passes = 0, dbg_index_spans = 0, dbg_index_whole = 0;
    // ... on a fresh index (index_parts_plan.h): the part jobs, the parts' pack table, lengths and statuses, the ranges'
    // records and slots; for flate_hip_debug_index_parts the direct and scratch parts of the last ranges call
    DevBuf ix_pjobs, ix_ptab, ix_plen, ix_pstatus, ix_rrec, ix_rdst;
    DevBuf ix_entries, ix_epack;  // flate_hip_index_scan: the walkers' lists as written and packed (jobs, records and the pack table lie in ix_jobs, ix_recs and ix_wtab)
    uint64_t dbg_index_direct = 0, dbg_index_scratch = 0;
    bool ws_fixed = false;   // the two-stream passes are being enqueued: ensure() may not grow a buffer (compress_impl)
    // last level 4..9 call, for the debug seam
    uint32_t dbg_pass_chunks = 0;
    uint32_t dbg_first_chunk = 0;
    std::vector<uint64_t> dbg_pos_off;
    std::vector<fl_chunk> dbg_chunks;   // whole-stream pass: chunk and piece tables of the last pass
    std::vector<fl_piece> dbg_pieces;
    // profiling
    bool prof = false;
    struct Pending {
        int kid;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> free_events;
    double prof_ms[K_COUNT] = {0};
    uint64_t prof_n[K_COUNT] = {0};
};

namespace {

#define HIP_OK(h, expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            (h)->last_error = std::string(#expr) + ": " + hipGetErrorString(e_);                         \
            return FLATE_HIP_E_LAUNCH;                                                                   \
        }                                                                                                \
    } while (0)

int ensure(flate_hip_ctx* h, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return FLATE_HIP_OK;
    if (h->ws_fixed) {
        // (the buffers may be slices of themselves and the second compute stream may still use them: never freed here)
        h->last_error = "workspace of the two-stream passes too small: " + std::to_string(bytes) + " bytes asked, " +
                        std::to_string(b.cap) + " held";
        return FLATE_HIP_E_LAUNCH;
    }
    if (b.p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(b.p);
        h->ws_bytes -= b.cap;
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // (the failure is answered here: a later HIP_OK(hipGetLastError()) must not see it)
        want = bytes;
        e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->last_error = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
        b.p = nullptr;
        return FLATE_HIP_E_ALLOC;
    }
    b.cap = want;
    h->ws_bytes += want;
    return FLATE_HIP_OK;
}

// ensure() for callers that have another way to go when there is no room: false, and the failure is not this call's
bool room(flate_hip_ctx* h, DevBuf& b, size_t bytes) {
    if (ensure(h, b, bytes) == FLATE_HIP_OK) return true;
    (void)hipGetLastError();
    return false;
}

// Pinned host memory of at least `want` bytes: what is there if it is large enough, else `sz` new bytes (the old ones are
// not kept).  false: no memory, the buffer is empty and the failure is answered here.
void pin_release(PinBuf& b) {
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}
bool pin_grow(PinBuf& b, size_t want, size_t sz) {
    if (want <= b.cap) return true;
    pin_release(b);
    if (hipHostMalloc(&b.p, sz, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return false;
    }
    b.cap = sz;
    return true;
}

// A side stream and the two events that tie it to the caller's stream: all three or none
bool side_stream(hipStream_t& s, hipEvent_t& ev0, hipEvent_t& ev1) {
    hipStream_t s_new = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipStreamCreateWithFlags(&s_new, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess) {
        s = s_new;
        ev0 = e0;
        ev1 = e1;
        return true;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s_new) (void)hipStreamDestroy(s_new);
    (void)hipGetLastError();
    return false;
}

// compute units of the device, asked once (256 where the device does not say)
uint32_t device_cu_count(flate_hip_ctx* h) {
    if (h->n_cu == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, h->device) != hipSuccess || v <= 0) v = 256;
        h->n_cu = (uint32_t)v;
    }
    return h->n_cu;
}

hipEvent_t get_event(flate_hip_ctx* h) {
    if (!h->free_events.empty()) {
        hipEvent_t e = h->free_events.back();
        h->free_events.pop_back();
        return e;
    }
    hipEvent_t e;
    (void)hipEventCreate(&e);
    return e;
}

struct ProfScope {
    flate_hip_ctx* h;
    int kid;
    hipStream_t s;
    hipEvent_t a{}, b{};
    ProfScope(flate_hip_ctx* h_, int kid_, hipStream_t s_ = nullptr) : h(h_), kid(kid_), s(s_ ? s_ : h_->stream) {
        if (h->prof) {
            a = get_event(h);
            b = get_event(h);
            (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (h->prof) {
            (void)hipEventRecord(b, s);
            h->pending.push_back({kid, a, b});
        }
    }
};

// k_checksum beside the kernels that follow on the compute stream; enqueue_back_end joins it
int launch_checksum_side(flate_hip_ctx* h, uint32_t nb, const uint8_t* d_in, const fl_chunk* dch, const uint32_t* dbc,
                         const fl_sblock* dsb, const fl_params& prm);

void fold_profile(flate_hip_ctx* h) {
    if (h->pending.empty()) return;
    (void)hipStreamSynchronize(h->stream);
    for (auto& p : h->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            h->prof_ms[p.kid] += ms;
            h->prof_n[p.kid] += 1;
        }
        h->free_events.push_back(p.a);
        h->free_events.push_back(p.b);
    }
    h->pending.clear();
}

void init_crc_consts(fl_crc_consts& cc) {
    cc.xpow8[0] = 0x00800000u;  // x^8 in the reflected representation (x^0 = 0x80000000)
    for (int j = 1; j < 32; j++) cc.xpow8[j] = fl_crc_mulmod(cc.xpow8[j - 1], cc.xpow8[j - 1]);
    for (int m = 0; m < 64; m++) cc.pow1024[m] = fl_crc_xpow8n(cc.xpow8, 1024ull * m);
    cc.pow65535 = fl_crc_xpow8n(cc.xpow8, 65535);
}

bool level_args(int mode, fl_params& p) {  // deflate.zig:41-52
    switch (mode) {
        case 4: p.good = 4; p.lazy = 4; p.nice = 16; p.chain = 16; return true;
        case 5: p.good = 8; p.lazy = 16; p.nice = 32; p.chain = 32; return true;
        case 6: p.good = 8; p.lazy = 16; p.nice = 128; p.chain = 128; return true;
        case 7: p.good = 8; p.lazy = 32; p.nice = 128; p.chain = 256; return true;
        case 8: p.good = 32; p.lazy = 128; p.nice = 258; p.chain = 1024; return true;
        case 9: p.good = 32; p.lazy = 258; p.nice = 258; p.chain = 4096; return true;
        default: p.good = p.lazy = p.nice = p.chain = 0; return mode == 0 || mode == 1;
    }
}

void read_knobs(fl_knobs& k, uint64_t span_default) {
    k = fl_knobs();
    const char* e;
    if ((e = getenv("FLATE_HIP_MAX_PASS_CHUNKS")) && atoi(e) > 0) k.max_pass_chunks = (size_t)atoi(e);
    if ((e = getenv("FLATE_HIP_HOST_PASS_CHUNKS")) && atoi(e) > 0) k.host_pass_chunks = (size_t)atoi(e);
    if ((e = getenv("FLATE_HIP_MAX_STREAM_PASS_MIB")) && atoll(e) > 0) k.stream_pass_bytes = (uint64_t)atoll(e) << 20;
    e = getenv("FLATE_HIP_INFLATE_SPANS");
    k.span_min_bytes = e ? (uint64_t)atoll(e) : span_default;
    k.span_debug = getenv("FLATE_HIP_SPAN_DEBUG") != nullptr;
    if ((e = getenv("FLATE_HIP_SPAN_TWIN"))) k.span_twin = atoi(e);
    k.no_pin_mirror = getenv("FLATE_HIP_NO_PIN_MIRROR") != nullptr;
    k.no_ramp = getenv("FLATE_HIP_NO_RAMP") != nullptr;
    if ((e = getenv("FLATE_HIP_RECT"))) k.rect = atoi(e) != 0;
    k.one_stream = getenv("FLATE_HIP_ONE_COMPUTE_STREAM") != nullptr;
    k.simple_ck_inline = getenv("FLATE_HIP_SIMPLE_CK_INLINE") != nullptr;
    if ((e = getenv("FLATE_HIP_SPAN_TWO_RUNS"))) k.span_two_runs = atoi(e) != 0;
    if ((e = getenv("FLATE_HIP_MEMSET_INLINE"))) k.memset_inline = atoi(e) != 0;
    if ((e = getenv("FLATE_HIP_STREAM_WINDOWS"))) k.stream_windows = atoi(e) != 0;
    if ((e = getenv("FLATE_HIP_STREAM_GROUP")) && atoi(e) > 0) k.stream_group = (uint32_t)atoi(e);
    if ((e = getenv("FLATE_HIP_INFLATE_PAR"))) k.inflate_par = atoll(e);
    if ((e = getenv("FLATE_HIP_INFLATE_RING"))) k.inflate_ring = atoll(e);
    if ((e = getenv("FLATE_HIP_MEMBER_SCAN"))) k.member_scan = atoi(e) != 0;
    if ((e = getenv("FLATE_HIP_INDEX_PASS_BYTES")) && atoll(e) > 0) k.index_pass_bytes = (uint64_t)atoll(e);
    if ((e = getenv("FLATE_HIP_MEMBER_CANDIDATES")) && atoll(e) >= 0 && atoll(e) <= 0x7fffffffll) k.member_candidates = (uint32_t)atoll(e);
}
bool is_pinned_host(const void* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // plain pageable memory: not an error of ours
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// The copy streams of the host-buffer paths.  HIP multiplexes the streams of one priority onto a few hardware queues (four by
// default), torch's and the caller's included, and two streams that land on one queue run IN ORDER: with the input stream and the
// output stream on one queue, the input copy of sub-batch k + 1 sits behind the output copy of k, which waits for the kernels of
// k -- nothing overlaps any more (rocprofv3 timeline, profiles/r05_host_path.txt: H2D 1.19 + kernels 2.15 + D2H 0.6 ms one after
// the other, 16.6 ms per 256 MiB instead of 10.4; which way a process went was luck).  Queues are pooled per PRIORITY: the
// input stream gets the highest, the output stream the lowest, the kernels stay on the caller's (normal): three pools.
hipError_t create_copy_stream(hipStream_t* s, bool input) {
    int least = 0, greatest = 0;  // (numerically: greatest priority = lowest number)
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) {
        (void)hipGetLastError();
        return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    }
    return hipStreamCreateWithPriority(s, hipStreamNonBlocking, input ? greatest : least);
}

int xfer_event(flate_hip_ctx* h, size_t k, hipEvent_t* ev) {
    while (h->xfer_events.size() <= k) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return FLATE_HIP_E_ALLOC;
        h->xfer_events.push_back(e);
    }
    *ev = h->xfer_events[k];
    return FLATE_HIP_OK;
}

// ---- Levels 4..9, whole-stream pass: the tokenizer kernels (kernels_stream.h).  What a pass does is decided in
// stream_plan.h; compress_stream_pass below carries it out, stage by stage, over one record per pass.
struct StreamPass {
    flate_hip_ctx* h;
    hipStream_t st;
    const uint8_t* d_in;
    const fl_params& prm;
    uint32_t nc, nb;
    const StreamTables& t;
    const fl_chunk* hch;  // the pass's chunks, host copy
    fl_stream_dims dims;
    bool windows = false;    // the pass is on the windows of k_lz_parse<true> / k_lz_walk<true, true> (until it gives them up)
    fl_stream_win win;       // ... its window and group tables
    uint32_t round_cap = 0;  // ... rounds of a window's stitch after which the pass is given to the tiles (0: never)
    // the tables on the device
    const fl_chunk* dch = nullptr;  // the streams
    const fl_chunk* dwc = nullptr;  // the windows
    const fl_seg* dsg = nullptr;
    const fl_piece* dpc = nullptr;
    const uint32_t* dfp = nullptr;
    uint32_t *d_wexit = nullptr, *d_gexit = nullptr, *d_gentry = nullptr, *d_dirty = nullptr;  // fl_wexit_layout
};

// the handle's buffer behind each name of stream_plan.h (in the order of fl_ws_buf)
DevBuf& stream_ws_buf(flate_hip_ctx* h, fl_ws_buf id) {
    DevBuf* const bufs[] = {&h->tiles,   &h->segs,  &h->pieces, &h->fpts,    &h->zones,   &h->nsorted, &h->cflag,
                            &h->S,       &h->desc,  &h->tokens, &h->marks,   &h->entry,   &h->segtok,  &h->tokbase,
                            &h->bound,   &h->ntok,  &h->wchunks, &h->swins,  &h->links,   &h->wexit,   &h->NC,
                            &h->rec,     &h->jmp,   &h->exitmap, &h->sgroups, &h->sgroup0, &h->gmap,   &h->gentry};
    static_assert(sizeof bufs / sizeof bufs[0] == FL_WS_COUNT, "a buffer per fl_ws_buf");
    return *bufs[id];
}
int ensure_stream_ws(flate_hip_ctx* h, const fl_ws_list& need) {
    int rc;
    for (uint32_t i = 0; i < need.n; i++)
        if ((rc = ensure(h, stream_ws_buf(h, need.v[i].buf), need.v[i].bytes))) return rc;
    return FLATE_HIP_OK;
}

// what every pass needs, reserved; its tables on the device; histograms and anchor bits cleared
int upload_stream_tables(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const StreamTables& t = sp.t;
    const uint32_t nseg = sp.dims.nseg, npc = sp.dims.npc;
    int rc;
    if ((rc = ensure_stream_ws(h, fl_stream_ws_common(sp.dims)))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->tiles.p, t.tiles.data(), sizeof(fl_tile) * t.tiles.size(), hipMemcpyHostToDevice, st));
    if (nseg) HIP_OK(h, hipMemcpyAsync(h->segs.p, t.segs.data(), sizeof(fl_seg) * nseg, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->pieces.p, t.pieces.data(), sizeof(fl_piece) * npc, hipMemcpyHostToDevice, st));
    if (!t.fpts.empty())
        HIP_OK(h, hipMemcpyAsync(h->fpts.p, t.fpts.data(), sizeof(uint32_t) * t.fpts.size(), hipMemcpyHostToDevice, st));
    if (!t.zones.empty())
        HIP_OK(h, hipMemcpyAsync(h->zones.p, t.zones.data(), sizeof(uint32_t) * t.zones.size(), hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemsetAsync(h->hist.p, 0, sizeof(uint32_t) * 320 * (size_t)sp.nb, st));
    HIP_OK(h, hipMemsetAsync(h->marks.p, 0, sp.dims.npos / 8, st));
    HIP_OK(h, hipStreamSynchronize(st));  // the host vectors must outlive the async copies
    sp.dch = (const fl_chunk*)h->chunks.p;
    sp.dsg = (const fl_seg*)h->segs.p;
    sp.dpc = (const fl_piece*)h->pieces.p;
    sp.dfp = (const uint32_t*)h->fpts.p;
    return FLATE_HIP_OK;
}

// windows or tiles (stream_plan.h: the rules and why); the one thing decided here is what only the device can say
void plan_stream_windows(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    const bool deep_walk = sp.dims.deep_walk;
    sp.windows = fl_stream_windows_allowed(sp.t.any_flush, deep_walk, h->knobs.stream_windows, sp.dims.nseg);
    if (!sp.windows) return;
    fl_stream_windows(sp.hch, sp.nc, h->knobs.stream_group, device_cu_count(h), deep_walk, sp.win);
    const fl_stream_choice choice = fl_stream_estimate(sp.win, sp.nc, deep_walk, h->knobs.stream_windows, h->knobs.max_pass_chunks);
    sp.round_cap = choice.round_cap;
    sp.windows = choice.windows;
    // (levels 8-9: a device that cannot give the windows' links: the tiles)
    if (sp.windows && deep_walk && !room(h, h->links, fl_stream_links_bytes((uint32_t)sp.win.wch.size()))) sp.windows = false;
}

// the windows' workspace, reserved; the window and group tables on the device
int upload_stream_windows(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const uint32_t nw = (uint32_t)sp.win.wch.size(), ng = (uint32_t)sp.win.sws.size();
    int rc;
    if ((rc = ensure_stream_ws(h, fl_stream_ws_windows(sp.dims, nw, ng)))) return rc;
    const fl_wexit_layout x = fl_wexit_offsets(nw, ng);
    sp.d_wexit = (uint32_t*)h->wexit.p + x.wexit;
    sp.d_gexit = (uint32_t*)h->wexit.p + x.gexit;
    sp.d_gentry = (uint32_t*)h->wexit.p + x.gentry;
    sp.d_dirty = (uint32_t*)h->wexit.p + x.dirty;
    HIP_OK(h, hipMemcpyAsync(h->wchunks.p, sp.win.wch.data(), sizeof(fl_chunk) * nw, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->swins.p, sp.win.sws.data(), sizeof(fl_swin) * ng, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));  // the host vectors must outlive the async copies
    sp.dwc = (const fl_chunk*)h->wchunks.p;
    return FLATE_HIP_OK;
}

// the tokenizer over the groups of windows: the first launch (fix = 0), or one from the groups' true entries (fix = 1)
void launch_stream_tokenizer(StreamPass& sp, uint32_t fix) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const uint32_t ng = (uint32_t)sp.win.sws.size();
    fix |= sp.round_cap << 8;
    if (sp.dims.deep_walk) {
        ProfScope ps(h, K_LZ_WALK);
        wk_stream ws{(const fl_swin*)h->swins.p, sp.dch, (const uint32_t*)h->zones.p, sp.d_gexit, sp.d_gentry, sp.d_wexit, sp.d_dirty, fix};
        hipLaunchKernelGGL((k_lz_walk<true, true>), dim3(ng), dim3(WK_THREADS), 0, st, sp.d_in, sp.dwc, sp.prm, (const uint16_t*)h->links.p,
                           (const uint32_t*)h->cflag.p, (uint32_t*)h->desc.p, (uint32_t*)h->marks.p, ws);
    } else {
        ProfScope ps(h, K_LZ_PARSE);
        hipLaunchKernelGGL(k_lz_parse<true>, dim3(ng), dim3(PZ_THREADS), 0, st, sp.d_in, sp.dwc, sp.prm,
                           (const uint16_t*)h->S.p, (const uint32_t*)h->cflag.p, (uint32_t*)h->desc.p, (uint32_t*)h->marks.p,
                           (const fl_swin*)h->swins.p, sp.dch, (const uint32_t*)h->zones.p, sp.d_gexit, sp.d_gentry, sp.d_wexit, sp.d_dirty, fix,
                           sp.t.any_flush ? sp.dfp : (const uint32_t*)nullptr);
    }
}

// the chains of every window: the four link arrays of levels 8-9, or the one of levels 4-7
void build_stream_chains(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const dim3 grid((uint32_t)sp.win.wch.size()), block(64 * FL_CHAIN_WAVES);
    if (sp.dims.deep_walk) {
        ProfScope ps(h, K_LZ_LINKS);
        void (*const links[4])(const uint8_t*, const fl_chunk*, uint16_t*, uint32_t*) = {k_lz_links<0>, k_lz_links<1>, k_lz_links<2>, k_lz_links<3>};
        for (auto k : links) hipLaunchKernelGGL(k, grid, block, 0, st, sp.d_in, sp.dwc, (uint16_t*)h->links.p, (uint32_t*)h->cflag.p);
    } else {
        ProfScope ps(h, K_LZ_CHAIN);
        if (sp.t.any_flush)
            hipLaunchKernelGGL(k_lz_chain<true>, grid, block, 0, st, sp.d_in, sp.dwc, (uint16_t*)h->S.p, (uint32_t*)h->cflag.p,
                               (uint32_t*)nullptr, sp.dfp);
        else
            hipLaunchKernelGGL(k_lz_chain<false>, grid, block, 0, st, sp.d_in, sp.dwc, (uint16_t*)h->S.p, (uint32_t*)h->cflag.p,
                               (uint32_t*)nullptr, (const uint32_t*)nullptr);
    }
}

// the dirty word behind the launch just enqueued, and what it means (fl_fix_verdict)
int read_fix_verdict(StreamPass& sp, uint32_t it, fl_fix& verdict) {
    flate_hip_ctx* h = sp.h;
    uint32_t flag = 0;
    HIP_OK(h, hipMemcpyAsync(&flag, sp.d_dirty, sizeof flag, hipMemcpyDeviceToHost, sp.st));
    HIP_OK(h, hipStreamSynchronize(sp.st));
    verdict = fl_fix_verdict(it, flag, (uint32_t)sp.win.sws.size());
    return FLATE_HIP_OK;
}

// The tokenizer over the windows, and for a grouped pass its fix launches until nothing moves any more.  A pass that gives
// up goes to the tiles (the anchors marked so far go); one that settles counts its segments' tokens.
int run_stream_windows(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    int rc;
    if ((rc = upload_stream_windows(sp))) return rc;
    build_stream_chains(sp);
    HIP_OK(h, hipMemsetAsync(sp.d_dirty, 0, sizeof(uint32_t), st));
    launch_stream_tokenizer(sp, 0u);
    fl_fix verdict;
    if ((rc = read_fix_verdict(sp, FL_FIX_FIRST, verdict))) return rc;
    for (uint32_t it = 0; sp.win.grouped && verdict == FL_FIX_AGAIN; it++) {
        HIP_OK(h, hipMemsetAsync(sp.d_dirty, 0, sizeof(uint32_t), st));
        launch_stream_tokenizer(sp, 1u);
        if ((rc = read_fix_verdict(sp, it, verdict))) return rc;
    }
    if (verdict == FL_FIX_GIVE_UP) {
        sp.windows = false;
        // (the tiles' sort scratch is what upload_stream_tables reserved: buffers only grow)
        HIP_OK(h, hipMemsetAsync(h->marks.p, 0, sp.dims.npos / 8, st));
    } else {
        ProfScope ps(h, K_ST_PARSE);
        hipLaunchKernelGGL(k_st_count, dim3(sp.dims.nseg), dim3(FL_PARSE_THREADS), 0, st, sp.dch, sp.dpc, sp.dsg, (const uint32_t*)h->desc.p,
                           (const uint32_t*)h->marks.p, (uint32_t*)h->segtok.p);
    }
    return FLATE_HIP_OK;
}

// sort / match over the 64 KiB tiles: a record for every position
int run_stream_tiles(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const StreamTables& t = sp.t;
    const size_t tiles_per_launch = sp.dims.tiles_per_launch;
    int rc;
    if ((rc = ensure_stream_ws(h, fl_stream_ws_tiles(sp.dims)))) return rc;
    // positions a flush keeps out of the hash table get no record from the match finder
    if (t.any_flush && hipMemsetAsync(h->rec.p, 0, fl_stream_rec_bytes(sp.dims.npos), st) != hipSuccess) return FLATE_HIP_E_LAUNCH;
    for (size_t t0 = 0; t0 < t.tiles.size(); t0 += tiles_per_launch) {
        const uint32_t nt = (uint32_t)std::min(tiles_per_launch, t.tiles.size() - t0);
        const fl_tile* dti = (const fl_tile*)h->tiles.p + t0;
        {
            ProfScope ps(h, K_LZ_SORT);
            hipLaunchKernelGGL(k_lz_sort<true>, dim3(nt), dim3(FL_SORT_THREADS), 0, st, sp.d_in, sp.dch, dti, sp.dfp,
                               (uint32_t*)h->nsorted.p, (uint16_t*)h->S.p,
                               (uint32_t*)h->cflag.p);
        }
        {
            ProfScope ps(h, K_LZ_MATCH);
            const uint32_t* cf = (const uint32_t*)h->cflag.p;
            hipLaunchKernelGGL((k_lz_match<true, true, false>), dim3(nt), dim3(FL_MATCH_THREADS), 0, st, sp.d_in, sp.dch, dti,
                               sp.dfp, (const uint32_t*)h->nsorted.p, sp.prm, (const uint16_t*)h->S.p, (uint32_t*)h->NC.p,
                               (uint32_t*)h->rec.p, cf);
            // the tiles k_lz_sort marked runny
            hipLaunchKernelGGL((k_lz_match<true, true, true>), dim3(nt), dim3(FL_MATCH_THREADS), 0, st, sp.d_in, sp.dch,
                               dti, sp.dfp, (const uint32_t*)h->nsorted.p, sp.prm, (const uint16_t*)h->S.p,
                               (uint32_t*)h->NC.p, (uint32_t*)h->rec.p, cf);
        }
    }
    return FLATE_HIP_OK;
}

// the walk from segment to segment over groups of segments (fl_stitch_plan: some piece is long)
int stitch_stream_groups(StreamPass& sp, const fl_stitch_tables& s) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const uint32_t npc = sp.dims.npc, ngr = (uint32_t)s.groups.size();
    int rc;
    if ((rc = ensure_stream_ws(h, fl_stream_ws_stitch(ngr, npc)))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->sgroups.p, s.groups.data(), sizeof(fl_sgroup) * ngr, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->sgroup0.p, s.group0.data(), sizeof(uint32_t) * npc, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));
    if (!ngr) return FLATE_HIP_OK;
    hipLaunchKernelGGL(k_st_stitch_a, dim3(ngr), dim3(FL_SEG_ENTRIES), 0, st, sp.dpc,
                       (const fl_sgroup*)h->sgroups.p, sp.dsg, (const uint16_t*)h->exitmap.p,
                       (uint16_t*)h->gmap.p);
    hipLaunchKernelGGL(k_st_stitch_b, dim3((npc + 63) / 64), dim3(64), 0, st, sp.dpc, npc,
                       (const uint32_t*)h->sgroup0.p, sp.dsg, (const uint16_t*)h->gmap.p,
                       (uint32_t*)h->gentry.p);
    hipLaunchKernelGGL(k_st_stitch_c, dim3((ngr + 63) / 64), dim3(64), 0, st, sp.dpc,
                       (const fl_sgroup*)h->sgroups.p, ngr, sp.dsg, (const uint16_t*)h->exitmap.p,
                       (const uint32_t*)h->gentry.p, (uint32_t*)h->entry.p);
    return FLATE_HIP_OK;
}

// the tiles' records into anchors: every segment for each entry it can be handed, the stitch, every segment from its own
int parse_stream_records(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const uint32_t nseg = sp.dims.nseg, npc = sp.dims.npc;
    int rc;
    ProfScope ps(h, K_ST_PARSE);
    hipLaunchKernelGGL(k_st_parse1, dim3(nseg), dim3(FL_PARSE_THREADS), 0, st, sp.dch, sp.dpc, sp.dsg, sp.prm,
                       (const uint32_t*)h->rec.p, (uint32_t*)h->desc.p, (uint16_t*)h->jmp.p,
                       (uint16_t*)h->exitmap.p);
    fl_stitch_tables stitch;
    fl_stitch_plan(sp.t.pieces.data(), npc, stitch);
    if (stitch.direct) {
        hipLaunchKernelGGL(k_st_stitch, dim3((npc + 63) / 64), dim3(64), 0, st, sp.dpc, npc, sp.dsg,
                           (const uint16_t*)h->exitmap.p, (uint32_t*)h->entry.p);
    } else if ((rc = stitch_stream_groups(sp, stitch))) {
        return rc;
    }
    hipLaunchKernelGGL(k_st_parse2, dim3(nseg), dim3(FL_PARSE_THREADS), 0, st, sp.dch, sp.dpc, sp.dsg,
                       (const uint32_t*)h->desc.p, (const uint16_t*)h->jmp.p, (const uint32_t*)h->entry.p,
                       (uint32_t*)h->marks.p, (uint32_t*)h->segtok.p);
    return FLATE_HIP_OK;
}

// tokens numbered through every piece, written with their histograms, cut into blocks
void emit_stream_tokens(StreamPass& sp) {
    flate_hip_ctx* h = sp.h;
    hipStream_t st = sp.st;
    const uint32_t nseg = sp.dims.nseg, npc = sp.dims.npc, nb = sp.nb;
    ProfScope ps(h, K_ST_EMIT);
    hipLaunchKernelGGL(k_st_scan, dim3(npc), dim3(64), 0, st, sp.dpc, (const uint32_t*)h->segtok.p,
                       (uint32_t*)h->tokbase.p, (uint32_t*)h->ntok.p);
    if (nseg)
        hipLaunchKernelGGL(k_st_emit, dim3(nseg), dim3(FL_EMIT_THREADS), 0, st, sp.d_in, sp.dch, sp.dpc, sp.dsg, sp.prm,
                           (const uint32_t*)h->desc.p, (const uint32_t*)h->marks.p,
                           (const uint32_t*)h->tokbase.p, (uint32_t*)h->tokens.p, (uint32_t*)h->hist.p,
                           (uint32_t*)h->bound.p, (uint32_t*)h->bound.p + nb);
    hipLaunchKernelGGL(k_st_blocks, dim3(npc), dim3(64), 0, st, sp.dch, sp.dpc, (const uint32_t*)h->ntok.p,
                       (const uint32_t*)h->bound.p, (const uint32_t*)h->bound.p + nb, sp.prm.flags & FL_PRM_REPAIR_Q1,
                       (const uint32_t*)h->zones.p, (fl_block_plan*)h->plans.p);
}

// Leaves tokens, histograms and the block table for the shared back end.
int compress_stream_pass(flate_hip_ctx* h, const uint8_t* d_in, const fl_params& prm, uint32_t nc, uint32_t nb,
                         const StreamTables& t, const fl_chunk* hch /* the pass's chunks, host copy */) {
    StreamPass sp{h, h->stream, d_in, prm, nc, nb, t, hch};
    sp.dims = fl_stream_dims_of(t, nb, h->knobs.max_pass_chunks, fl_stream_deep_walk(prm.chain));
    int rc;
    if ((rc = upload_stream_tables(sp))) return rc;
    plan_stream_windows(sp);
    if (sp.windows && (rc = run_stream_windows(sp))) return rc;  // (may hand the pass to the tiles)
    if (!sp.windows) {
        if ((rc = run_stream_tiles(sp))) return rc;
        if (sp.dims.nseg && (rc = parse_stream_records(sp))) return rc;
    }
    emit_stream_tokens(sp);
    return FLATE_HIP_OK;
}

// k_gather_copy: about 4096 workgroups whatever the number of streams (one long stream is cut into slices)
dim3 gather_grid(uint32_t n) { return dim3(n, std::max(1u, std::min(1024u, 4096u / std::max(n, 1u)))); }

// n values of a caller's array to the host (memkind says where they are)
template <class T>
int fetch_array(flate_hip_ctx* h, const T* p, uint64_t n, int memkind, std::vector<T>& host) {
    host.resize(n);
    if (!n) return FLATE_HIP_OK;
    if (memkind == FLATE_HIP_MEM_HOST) {
        memcpy(host.data(), p, sizeof(T) * n);
    } else {
        HIP_OK(h, hipMemcpyAsync(host.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost, h->stream));
        HIP_OK(h, hipStreamSynchronize(h->stream));
    }
    return FLATE_HIP_OK;
}

// Fetch the n+1 offsets to the host (the block tables are built there); they may not go backwards.
int fetch_offsets(flate_hip_ctx* h, const uint64_t* off, uint32_t n, int memkind, std::vector<uint64_t>& host) {
    const int rc = fetch_array(h, off, (uint64_t)n + 1, memkind, host);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (host[i + 1] < host[i]) return FLATE_HIP_E_INVALID_ARG;
    return FLATE_HIP_OK;
}

// ---- The frame of the inflate entry points (decompress_core, the dict batch, the size probe, members, ranges): what the
// kernels of a call read and write.  Device memory: the caller's own buffers.  Host memory: staged twins in the handle's
// st_* buffers, whose offsets start at the caller's first byte (the two shifts); the results go home when the call ends.
// What the calls decide is inflate_plan.h's.
struct InflateFrame {
    flate_hip_ctx* h;
    bool host;   // memkind == FLATE_HIP_MEM_HOST
    uint32_t n;  // streams (ranges: ranges)
    uint64_t in_lo = 0, in_hi = 0, out_lo = 0, out_hi = 0;  // the caller's bytes, as offsets into its buffers (no output buffer: 0, 0)
    // the views (until stage_frame: the caller's pointers)
    const uint8_t* d_in = nullptr;
    uint8_t* d_out = nullptr;
    uint64_t* d_outlen = nullptr;
    int32_t* d_status = nullptr;
    uint64_t* d_consumed = nullptr;
    uint64_t in_shift = 0, out_shift = 0;  // what the views' offsets are less than the caller's

    InflateFrame(flate_hip_ctx* h_, int memkind, uint32_t n_) : h(h_), host(memkind == FLATE_HIP_MEM_HOST), n(n_) {}
    InflateFrame& input(const uint8_t* in, uint64_t lo, uint64_t hi) {
        d_in = in, in_lo = lo, in_hi = hi;
        return *this;
    }
    InflateFrame& output(uint8_t* out, uint64_t lo, uint64_t hi) {
        d_out = out, out_lo = lo, out_hi = hi;
        return *this;
    }
    InflateFrame& results(uint64_t* out_len, int32_t* status, uint64_t* consumed) {
        d_outlen = out_len, d_status = status, d_consumed = consumed;
        return *this;
    }
};
// what a call stages beside in / out_len / status
enum : uint32_t {
    FRAME_OUT = 1,            // an output buffer
    FRAME_CONSUMED = 2,       // consumed ...
    FRAME_NULL_CONSUMED = 4,  // ... but the kernels see nullptr when the caller passed nullptr (else the staged array)
};

// host memory: the staging buffers of the call, at least as large as it needs them (nothing is copied yet)
int reserve_frame(const InflateFrame& f, uint32_t what) {
    if (!f.host) return FLATE_HIP_OK;
    flate_hip_ctx* h = f.h;
    int rc;
    if ((rc = ensure(h, h->st_in, (f.in_hi - f.in_lo) + 16))) return rc;
    if ((what & FRAME_OUT) && (rc = ensure(h, h->st_out, (f.out_hi - f.out_lo) + 16))) return rc;
    if ((rc = ensure(h, h->st_outlen, sizeof(uint64_t) * f.n))) return rc;
    if ((rc = ensure(h, h->st_status, sizeof(int32_t) * f.n))) return rc;
    if ((what & FRAME_CONSUMED) && (rc = ensure(h, h->st_consumed, sizeof(uint64_t) * f.n))) return rc;
    return FLATE_HIP_OK;
}

// host memory: the input bytes [iv[0], iv[1]), [iv[2], iv[3]), ... (the caller's offsets) go to their places in st_in --
// the whole input, the intervals a ranges call can consume, or nothing (the pinned path copies sub-batch by sub-batch) --
// and the views become the staged twins.
int stage_frame(InflateFrame& f, uint32_t what, const uint64_t* iv, size_t n_iv) {
    if (!f.host) return FLATE_HIP_OK;
    flate_hip_ctx* h = f.h;
    for (size_t k = 0; k + 1 < n_iv; k += 2)
        HIP_OK(h, hipMemcpyAsync((uint8_t*)h->st_in.p + (iv[k] - f.in_lo), f.d_in + iv[k], iv[k + 1] - iv[k], hipMemcpyHostToDevice,
                                 h->stream));
    f.d_in = (const uint8_t*)h->st_in.p;
    if (what & FRAME_OUT) f.d_out = (uint8_t*)h->st_out.p;
    f.d_outlen = (uint64_t*)h->st_outlen.p;
    f.d_status = (int32_t*)h->st_status.p;
    if (what & FRAME_CONSUMED) f.d_consumed = (f.d_consumed || !(what & FRAME_NULL_CONSUMED)) ? (uint64_t*)h->st_consumed.p : nullptr;
    f.in_shift = f.in_lo;
    f.out_shift = f.out_lo;
    return FLATE_HIP_OK;
}
// ... the whole input
int stage_frame_whole(InflateFrame& f, uint32_t what) {
    const uint64_t whole[2] = {f.in_lo, f.in_hi};
    return stage_frame(f, what, whole, f.in_hi > f.in_lo ? 2 : 0);
}

// (what goes back to a host caller beyond out_len[i] is zeros, never bytes of an earlier call; the copies of the
// call before are done: it waited for them)
int clear_staged_out(const InflateFrame& f) {
    if (f.host && f.out_hi > f.out_lo) HIP_OK(f.h, hipMemsetAsync(f.h->st_out.p, 0, f.out_hi - f.out_lo, f.h->stream));
    return FLATE_HIP_OK;
}

// the call's chunk table to the device; the host waits for it (the table is the caller's to change or drop)
int upload_chunks(flate_hip_ctx* h, const std::vector<fl_chunk>& chunks) {
    int rc;
    if ((rc = ensure(h, h->chunks, sizeof(fl_chunk) * chunks.size()))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->chunks.p, chunks.data(), sizeof(fl_chunk) * chunks.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(h, hipStreamSynchronize(h->stream));
    return FLATE_HIP_OK;
}

// The call ends: a host caller's out_len / status / consumed (where it asked for it) are sent home ...
int results_home(const InflateFrame& f, uint64_t* out_len, int32_t* status, uint64_t* consumed) {
    flate_hip_ctx* h = f.h;
    if (!f.host) return FLATE_HIP_OK;
    HIP_OK(h, hipMemcpyAsync(out_len, f.d_outlen, sizeof(uint64_t) * f.n, hipMemcpyDeviceToHost, h->stream));
    HIP_OK(h, hipMemcpyAsync(status, f.d_status, sizeof(int32_t) * f.n, hipMemcpyDeviceToHost, h->stream));
    if (consumed) HIP_OK(h, hipMemcpyAsync(consumed, f.d_consumed, sizeof(uint64_t) * f.n, hipMemcpyDeviceToHost, h->stream));
    return FLATE_HIP_OK;
}
// ... and the host waits for them; a device caller is waited for when the handle is synchronous
int wait_for_results(const InflateFrame& f) {
    if (f.host || f.h->sync) HIP_OK(f.h, hipStreamSynchronize(f.h->stream));
    return FLATE_HIP_OK;
}

// The produced bytes of n slots packed on the device (k_gather_copy), across PCIe once, and put into their slots by the
// host; the caller's bytes beyond out_len[i] are not touched.  hout: the slots' offsets in `out` (the caller's); total: the
// sum of out_len.  d_slot: the slots' offsets in d_out where the device has them already (ranges: the pack kernel's
// table) -- the packed offsets are then summed here and uploaded; nullptr: hout less out_shift is uploaded and the packed
// offsets are summed on the device (k_scan_lens).
int copy_out_packed(flate_hip_ctx* h, const uint8_t* d_out, const uint64_t* d_slot, const uint64_t* d_outlen, uint32_t n,
                    const std::vector<uint64_t>& hout, uint64_t out_shift, uint8_t* out, const uint64_t* out_len, uint64_t total) {
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure(h, h->st_pack, total + 16))) return rc;
    if ((rc = ensure(h, h->st_packoff, sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
    std::vector<uint64_t> tab((size_t)n + 1, 0);
    if (d_slot) {
        for (uint32_t i = 0; i < n; i++) tab[i + 1] = tab[i] + out_len[i];
        HIP_OK(h, hipMemcpyAsync(h->st_packoff.p, tab.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    } else {
        if ((rc = ensure(h, h->st_slot, sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
        for (uint32_t i = 0; i <= n; i++) tab[i] = hout[i] - out_shift;
        HIP_OK(h, hipMemcpyAsync(h->st_slot.p, tab.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, st, d_outlen, n, (uint64_t*)h->st_packoff.p);
        d_slot = (const uint64_t*)h->st_slot.p;
    }
    hipLaunchKernelGGL(k_gather_copy, gather_grid(n), dim3(256), 0, st, d_out, d_slot, d_outlen, (uint8_t*)h->st_pack.p,
                       (const uint64_t*)h->st_packoff.p);
    HIP_OK(h, hipGetLastError());
    std::vector<uint8_t> packed(total);
    HIP_OK(h, hipMemcpyAsync(packed.data(), h->st_pack.p, total, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (out_len[i]) memcpy(out + hout[i], packed.data() + at, out_len[i]);
        at += out_len[i];
    }
    return FLATE_HIP_OK;
}

// Host-buffer calls: bring back only what was produced (fl_copy_out_plan): packed, or the range up to the last produced
// byte as it is -- bytes of a slot beyond out_len[i] are then whatever the staging buffer held there (the callers clear it:
// zeros), in the packed case they are not touched.
int copy_out_host(flate_hip_ctx* h, const uint8_t* d_out, const uint64_t* d_outlen, uint32_t n,
                  const std::vector<uint64_t>& hout, uint64_t out_shift, uint8_t* out, const uint64_t* out_len) {
    const fl_copy_out p = fl_copy_out_plan(hout.data(), out_len, n);
    if (p.kind == FL_COPY_OUT_PACKED) return copy_out_packed(h, d_out, nullptr, d_outlen, n, hout, out_shift, out, out_len, p.total);
    if (p.kind == FL_COPY_OUT_DENSE) {
        const uint64_t out_lo = hout[0];
        HIP_OK(h, hipMemcpyAsync(out + out_lo, d_out + (out_lo - out_shift), p.end - out_lo, hipMemcpyDeviceToHost, h->stream));
        HIP_OK(h, hipStreamSynchronize(h->stream));
    }
    return FLATE_HIP_OK;
}

int decompress_core(flate_hip_ctx* h, const uint8_t* in, const std::vector<uint64_t>& hin, uint32_t n_chunks, int container,
                    int flags, uint8_t* out, const std::vector<uint64_t>& hout, uint64_t* out_len, int32_t* status,
                    uint64_t* consumed, int memkind);
struct SpanRecords;
int sizes_impl(flate_hip_ctx* h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks, int container, int flags,
               uint64_t* sizes, int32_t* status, uint64_t* consumed, int memkind, SpanRecords* keep);

// workspace of a chunk-path pass of nc chunks (levels 4..9)
// (pass_plan.h: the bytes per chunk of every buffer)
int ensure_lz_workspace(flate_hip_ctx* h, uint32_t nc, uint32_t chain) {
    int rc;
    const bool bulk = chain >= FL_BULK_MIN_CHAIN;
    const fl_lz_sizes z = fl_lz_chunk_sizes(bulk);
    if ((rc = ensure(h, bulk ? h->links : h->S, z.links * nc))) return rc;  // [L4 | L6 | L8 | RK] a chunk (kernels_walk.h) / chain links (kernels_parse.h)
    if ((rc = ensure(h, h->desc, z.desc * nc))) return rc;                 // anchor descriptors
    if ((rc = ensure(h, h->marks, z.marks * nc))) return rc;               // true anchors, one bit per position
    if ((rc = ensure(h, h->tokens, z.tokens * nc))) return rc;
    if ((rc = ensure(h, h->ntok, z.ntok * nc))) return rc;
    if ((rc = ensure(h, h->cflag, z.cflag * nc))) return rc;
    return FLATE_HIP_OK;
}
// plans, histograms and checksum words of a chunk-path pass of nb block slots (pass_plan.h)
int ensure_block_workspace(flate_hip_ctx* h, uint64_t nb) {
    int rc;
    const fl_blk_sizes b = fl_block_slot_sizes();
    if ((rc = ensure(h, h->plans, b.plan * nb))) return rc;
    if ((rc = ensure(h, h->hist, b.hist * nb))) return rc;
    return ensure(h, h->cks, b.cks * nb);
}

// shared back end of every pass: block planner, offset scan, bit packer
int launch_checksum_side(flate_hip_ctx* h, uint32_t nb, const uint8_t* d_in, const fl_chunk* dch, const uint32_t* dbc,
                         const fl_sblock* dsb, const fl_params& prm) {
    hipStream_t st = h->stream;
    if (!h->s_ck) {  // (all three or none: a half-made set would be skipped by every later call)
        hipStream_t s = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
            if (s) (void)hipStreamDestroy(s);
            (void)hipGetLastError();
            return FLATE_HIP_E_ALLOC;
        }
        h->s_ck = s;
        h->ck_ev0 = e0;
        h->ck_ev1 = e1;
    }
    // behind everything enqueued so far (the pass's tables and input, the kernels that read the checksums of the pass before)
    HIP_OK(h, hipEventRecord(h->ck_ev0, st));
    HIP_OK(h, hipStreamWaitEvent(h->s_ck, h->ck_ev0, 0));
    {
        ProfScope ps(h, K_CHECKSUM, h->s_ck);
        hipLaunchKernelGGL(k_checksum, dim3(nb), dim3(64), 0, h->s_ck, d_in, dch, dbc, dsb, prm, h->crc, (uint32_t*)h->cks.p);
    }
    HIP_OK(h, hipEventRecord(h->ck_ev1, h->s_ck));
    h->ck_pending = true;
    return FLATE_HIP_OK;
}

#ifndef FL_ENC_WAVE_MIN_SLOTS_STREAM
#define FL_ENC_WAVE_MIN_SLOTS_STREAM 32768u
#endif
int enqueue_back_end(flate_hip_ctx* h, const fl_params& prm, uint32_t nc, uint32_t nb, uint32_t c0, const fl_chunk* dch,
                     const uint32_t* dbc, const fl_sblock* dsb, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_outlen,
                     int32_t* d_status) {
    hipStream_t st = h->stream;
    const int mode = prm.mode;
    fl_block_plan* dpl = (fl_block_plan*)h->plans.p;
    uint32_t* dhist = (uint32_t*)h->hist.p;
    uint32_t* dcks = (uint32_t*)h->cks.p;
    {
        ProfScope ps(h, K_PLAN);
        if (mode == 0)
            hipLaunchKernelGGL(k_plan_store, dim3((nb + 255) / 256), dim3(256), 0, st, dch, dbc, dsb, nb, dpl);
        else
            hipLaunchKernelGGL(k_plan, dim3((nb + FL_PLAN_WAVES - 1) / FL_PLAN_WAVES), dim3(64 * FL_PLAN_WAVES), 0, st,
                               dch, dbc, dsb, prm, (const uint32_t*)dhist, dpl);
    }
    if (h->ck_pending) {  // the checksums of this pass (launch_checksum_side)
        HIP_OK(h, hipStreamWaitEvent(st, h->ck_ev1, 0));
        h->ck_pending = false;
    }
    if (h->ms_pending) {  // the output slots have been cleared (compress_impl)
        HIP_OK(h, hipStreamWaitEvent(st, h->ms_ev1, 0));
        h->ms_pending = false;
    }
    {
        ProfScope ps(h, K_OFFSETS);
        // (a wave per chunk; sixteen when the chunks are long streams of many blocks: config #4's one stream has 2049)
        hipLaunchKernelGGL(k_offsets, dim3(nc), dim3((uint64_t)nb >= 32ull * nc ? 64 * FL_OFFS_MAX_WAVES : 64), 0, st, dch, prm, h->crc, dpl, (const uint32_t*)dcks,
                           d_out, d_outlen + c0, d_status + c0);
    }
    {
        ProfScope ps(h, K_ENCODE);
        // many blocks (the chunk path: two plan slots per chunk): a wave per block, one pass over its tokens; few blocks
        // (long streams): a workgroup per block, its waves share the block
        // (whole-stream passes: a block holds 32768 tokens and most slots are empty -- 256 streams of 1 MiB have 3072 blocks in 8448
        // slots: four waves a block are faster than one until the blocks are many)
        if (mode >= 4 && nb >= (prm.stream ? FL_ENC_WAVE_MIN_SLOTS_STREAM : 8192u))
            hipLaunchKernelGGL(k_encode_wave, dim3((nb + FL_ENC_WAVES - 1) / FL_ENC_WAVES), dim3(64 * FL_ENC_WAVES), 0, st,
                               d_in, dch, dbc, (const fl_block_plan*)dpl, (const uint32_t*)h->tokens.p, (uint32_t*)d_out, nb,
                               (prm.stream || (nb & 1u)) ? 0u : 1u);
        else if (mode >= 4)
            hipLaunchKernelGGL(k_encode<true>, dim3(nb), dim3(64 * FL_ENC_WAVES), 0, st, d_in, dch, dbc,
                               (const fl_block_plan*)dpl, (const uint32_t*)h->tokens.p, (uint32_t*)d_out);
        else
            hipLaunchKernelGGL(k_encode<false>, dim3(nb), dim3(64 * FL_ENC_WAVES), 0, st, d_in, dch, dbc,
                               (const fl_block_plan*)dpl, (const uint32_t*)nullptr, (uint32_t*)d_out);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// flate_hip_compress_joined: behind the back end of a pass of pieces, on the pass's stream and over the pass's slice of the
// workspace -- the plans still hold the pass's blocks.  The pass took the joined container's checksum, a unit per piece, where
// every pass takes its checksum (enqueue_pass); the pieces are raw streams, so k_offsets left it alone: k_join_open moves it out.
int enqueue_join_open(flate_hip_ctx* h, const fl_params& prm, uint32_t nc, uint32_t nb, uint32_t c0, const fl_chunk* dch,
                      uint8_t* d_out, uint64_t* d_outlen, int32_t* d_status) {
    const JoinCall& jc = *h->join;
    hipStream_t st = h->stream;
    {
        ProfScope ps(h, K_JOIN_OPEN);
        hipLaunchKernelGGL(k_join_open, dim3((nc + 255) / 256), dim3(256), 0, st, dch, (const fl_block_plan*)h->plans.p, nc, c0,
                           jc.d_piece_stream, jc.d_streams, d_out, d_outlen, d_status,
                           jc.container != 0 ? (const uint32_t*)h->cks.p : (const uint32_t*)nullptr, jc.d_piece_cks);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// one pass of the chunk path (levels 4..9, inputs <= 65535 bytes) or of a simple mode: checksums,
// tokenizer / histograms, back end.  Only enqueues.
int enqueue_pass(flate_hip_ctx* h, const fl_params& prm, uint32_t nc, uint32_t nb, uint32_t c0, const fl_chunk* dch,
                 const uint32_t* dbc, const fl_sblock* dsb, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_outlen,
                 int32_t* d_status) {
    hipStream_t st = h->stream;
    // (the pieces of a joined call are raw chunks, and the pass takes the checksum of the container they are joined in: ckp)
    const int mode = prm.mode, container = h->join ? h->join->container : prm.container;
    fl_params ckp = prm;
    ckp.container = container;
    int rc;
    fl_block_plan* dpl = (fl_block_plan*)h->plans.p;
    uint32_t* dhist = (uint32_t*)h->hist.p;
    // The container's checksum reads the input and nothing else.  Levels 4-7: on a stream of its own beside k_lz_parse, which
    // lives in LDS (1 GiB gzip level 6: 30.1 -> 29.5 ms; the tokenizer pays 1.1 ms for a neighbour that takes 1.8) -- not
    // beside k_lz_chain (2.98 ms instead of 1.26 with the checksum next to it) and not beside k_lz_walk, whose gathers
    // wait for the same memory system (config #3: 9.95 -> 11.9 ms): there it runs first, on the compute stream.
    if (container != 0 && ((mode >= 4 && prm.chain >= FL_BULK_MIN_CHAIN) || (mode < 4 && h->knobs.simple_ck_inline))) {
        ProfScope ps(h, K_CHECKSUM);
        hipLaunchKernelGGL(k_checksum, dim3(nb), dim3(64), 0, st, d_in, dch, dbc, dsb, ckp, h->crc, (uint32_t*)h->cks.p);
    }
    // simple modes: beside the histograms and the planner, which are short chains of latency (config #4: 0.15 of 1.2 ms in line)
    if (container != 0 && mode < 4 && !h->knobs.simple_ck_inline && (rc = launch_checksum_side(h, nb, d_in, dch, dbc, dsb, ckp))) return rc;
    if (mode >= 4) {
        if ((rc = ensure_lz_workspace(h, nc, prm.chain))) return rc;
        if (prm.chain >= FL_BULK_MIN_CHAIN) {
            HIP_OK(h, hipMemsetAsync(h->marks.p, 0, fl_lz_chunk_sizes(true).marks * nc, st));  // k_lz_walk stores the anchors in (k_lz_chain clears its chunk's itself)
            // levels 8 and 9 (chains of 1024 / 4096 candidates): the reference's chain and two sparser ones in global
            // memory, the automaton over them (kernels_walk.h): a walk is 1.4 steps per byte instead of 14
            {
                ProfScope ps(h, K_LZ_LINKS);
                hipLaunchKernelGGL(k_lz_links<0>, dim3(nc), dim3(64 * FL_CHAIN_WAVES), 0, st, d_in, dch, (uint16_t*)h->links.p,
                                   (uint32_t*)h->cflag.p);
                hipLaunchKernelGGL(k_lz_links<1>, dim3(nc), dim3(64 * FL_CHAIN_WAVES), 0, st, d_in, dch, (uint16_t*)h->links.p,
                                   (uint32_t*)h->cflag.p);
                hipLaunchKernelGGL(k_lz_links<2>, dim3(nc), dim3(64 * FL_CHAIN_WAVES), 0, st, d_in, dch, (uint16_t*)h->links.p,
                                   (uint32_t*)h->cflag.p);
                hipLaunchKernelGGL(k_lz_links<3>, dim3(nc), dim3(64 * FL_CHAIN_WAVES), 0, st, d_in, dch, (uint16_t*)h->links.p,
                                   (uint32_t*)h->cflag.p);
            }
            {
                ProfScope ps(h, K_LZ_WALK);
                hipLaunchKernelGGL(k_lz_walk<false>, dim3(nc), dim3(WK_THREADS), 0, st, d_in, dch, prm, (const uint16_t*)h->links.p,
                                   (const uint32_t*)h->cflag.p, (uint32_t*)h->desc.p, (uint32_t*)h->marks.p, wk_stream{});
                // the chunks k_lz_links<0> found a run of one byte in (workgroups of the other kind return at once)
                hipLaunchKernelGGL(k_lz_walk<true>, dim3(nc), dim3(WK_THREADS), 0, st, d_in, dch, prm, (const uint16_t*)h->links.p,
                                   (const uint32_t*)h->cflag.p, (uint32_t*)h->desc.p, (uint32_t*)h->marks.p, wk_stream{});
            }
        } else {
            // levels 4..7: the reference's chain in LDS, the automaton per segment (kernels_parse.h)
            {
                ProfScope ps(h, K_LZ_CHAIN);
                hipLaunchKernelGGL(k_lz_chain<false>, dim3(nc), dim3(64 * FL_CHAIN_WAVES), 0, st, d_in, dch, (uint16_t*)h->S.p,
                                   (uint32_t*)h->cflag.p, (uint32_t*)h->marks.p, (const uint32_t*)nullptr);
            }
            if (container != 0 && (rc = launch_checksum_side(h, nb, d_in, dch, dbc, dsb, ckp))) return rc;
            {
                ProfScope ps(h, K_LZ_PARSE);
                hipLaunchKernelGGL(k_lz_parse<false>, dim3(nc), dim3(PZ_THREADS), 0, st, d_in, dch, prm, (const uint16_t*)h->S.p,
                                   (const uint32_t*)h->cflag.p, (uint32_t*)h->desc.p, (uint32_t*)h->marks.p,
                                   (const fl_swin*)nullptr, (const fl_chunk*)nullptr, (const uint32_t*)nullptr,
                                   (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (const uint32_t*)nullptr);
            }
        }
        {
            ProfScope ps(h, K_LZ_EMIT);
            hipLaunchKernelGGL(k_lz_emit, dim3(nc), dim3(FL_EMITZ_THREADS), 0, st, d_in, dch, prm,
                               (const uint32_t*)h->desc.p, (const uint32_t*)h->marks.p, (uint32_t*)h->tokens.p, dhist,
                               dpl, (uint32_t*)h->ntok.p);
        }
        h->dbg_pass_chunks = nc;
        h->dbg_first_chunk = c0;
        h->dbg_pos_off.resize(nc);
        h->dbg_pieces.clear();
        for (uint32_t i = 0; i < nc; i++) h->dbg_pos_off[i] = (uint64_t)i * FL_CHUNK_STRIDE;
    } else if (mode == 1) {
        ProfScope ps(h, K_BYTE_HIST);
        hipLaunchKernelGGL(k_byte_hist, dim3(nb), dim3(256), 0, st, d_in, dch, dbc, dsb, dhist);
    }
    if ((rc = enqueue_back_end(h, prm, nc, nb, c0, dch, dbc, dsb, d_in, d_out, d_outlen, d_status)) || !h->join) return rc;
    return enqueue_join_open(h, prm, nc, nb, c0, dch, d_out, d_outlen, d_status);
}


// k_span_scan over `points`: found[j] is the block start it found for points[j], on the host when this returns (one host
// wait).  Returns 1, or 0 when there is no room for the scan's buffers (the caller decodes every stream whole), or -1
// (a HIP call failed).
int scan_block_starts(flate_hip_ctx* h, hipStream_t st, const uint8_t* d_in, int flags, const std::vector<fl_scan_point>& points,
                      std::vector<uint64_t>& found) {
    const uint32_t npts = (uint32_t)points.size();
    if (!room(h, h->sp_points, sizeof(fl_scan_point) * npts) || !room(h, h->sp_found, sizeof(uint64_t) * npts)) return 0;
    if (hipMemcpyAsync(h->sp_points.p, points.data(), sizeof(fl_scan_point) * npts, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    {
        ProfScope ps(h, K_SPAN_SCAN);
        hipLaunchKernelGGL(k_span_scan, dim3(npts), dim3(FP_THREADS), 0, st, d_in, (const fl_chunk*)h->chunks.p, flags,
                           (const fl_scan_point*)h->sp_points.p, (uint64_t*)h->sp_found.p);
    }
    found.resize(npts);
    if (hipMemcpyAsync(found.data(), h->sp_found.p, sizeof(uint64_t) * npts, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    return 1;
}

// FLATE_HIP_SPAN_DEBUG: what the walk over one stream's records (span_plan.h, fl_span_follow_chain) saw and made of them
void span_debug_chain(const fl_span_chain& pl, uint32_t stream, const std::vector<fl_span>& spans, const std::vector<fl_span_res>& r1,
                      uint32_t a, uint32_t b) {
    std::vector<uint32_t> seen = pl.chain;
    if (seen.empty() || seen.back() != pl.last) seen.push_back(pl.last);  // (the span whose record ended the walk before it joined)
    for (size_t g = 0; g < seen.size() && g < 6; g++) {
        const fl_span_res& r = r1[seen[g]];
        fprintf(stderr, "[spans] pass 1 span %u: start %llu status %u end %llu out %llu final %u\n", seen[g], (unsigned long long)spans[seen[g]].start_bit, r.status, (unsigned long long)r.end_bit, (unsigned long long)r.out_len, r.final_seen);
    }
    fprintf(stderr, "[spans] stream %u: chain of %zu spans, %llu bytes, ok=%d\n", stream, pl.chain.size(), (unsigned long long)pl.total, (int)pl.ok);
    for (uint32_t j = a; j < b; j++)
        fprintf(stderr, "[spans]    span %u: start %llu status %u (0: decoded; else why it gave up) end %llu out %llu final %u blocks / pieces %u\n", j,
                (unsigned long long)spans[j].start_bit, r1[j].status, (unsigned long long)r1[j].end_bit, (unsigned long long)r1[j].out_len, r1[j].final_seen, r1[j].n_pieces);
}

// Long streams, few of them: cut each at block starts into spans and decode the spans at once, twice
// (kernels_inflate_par.h, "spans").  Streams that come out whole get their status / out_len / consumed here and
// chunks[i].skip = 1 (the kernels that follow leave them alone); everything else stays as it was.
// Every decision is span_plan.h's; this is plan, upload, launch, read back, three times (three host waits).
// No room for a buffer: 0, the old way.  Returns the number of streams finished, or a negative FLATE_HIP_E_*.
int try_span_inflate(flate_hip_ctx* h, hipStream_t st, const uint8_t* d_in, std::vector<fl_chunk>& chunks, int container,
                     int flags, uint8_t* d_out, uint64_t* d_outlen, int32_t* d_status, uint64_t* d_consumed) {
    const uint32_t n_chunks = (uint32_t)chunks.size();
    const uint64_t min_bytes = h->knobs.span_min_bytes;  // FLATE_HIP_INFLATE_SPANS -- 0: never; else the minimum stream size in bytes
    const bool dbg = h->knobs.span_debug;
    const auto t_begin = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); };
    const uint32_t n_cu = device_cu_count(h);
    const int etw = h->knobs.span_twin;  // FLATE_HIP_SPAN_TWIN -- -1: unset; 0: never; 2..950: where to cut, in thousandths of the stream (tuning)
    const bool sym = !h->knobs.span_two_runs;  // one decode per span, in symbols (kernels_inflate_par.h)
    const fl_span_elig taken = fl_span_eligible(chunks.data(), n_chunks, min_bytes, flags, n_cu, etw);
    const std::vector<uint32_t>& elig = taken.elig;
    const bool twin = taken.twin;
    const bool both = twin || sym;  // what run B makes is there after run A's launch
    if (elig.empty()) return 0;
    h->dbg_span_taken = elig.size();  // (what does not come out whole below is handed on)
    // ---- where spans may start
    std::vector<fl_scan_point> points;
    std::vector<uint32_t> pt_first;
    fl_span_targets(chunks.data(), elig, twin, etw, sym, n_cu, points, pt_first);
    const uint32_t npts = (uint32_t)points.size();
    std::vector<uint64_t> found;
    if (const int sc = scan_block_starts(h, st, d_in, flags, points, found); sc <= 0) return sc;
    const fl_chunk* dch = (const fl_chunk*)h->chunks.p;
    if (dbg) fprintf(stderr, "[spans] %.3f ms: sync 1 done\n", since());
    // ---- the spans: the stream start, then every distinct position found
    std::vector<fl_span> spans;
    std::vector<uint64_t> cand;
    std::vector<uint32_t> cand_off, sp_first;
    fl_span_build(n_chunks, elig, pt_first, found.data(), spans, cand, cand_off, sp_first);
    const uint32_t nsp = (uint32_t)spans.size();
    if (dbg) fprintf(stderr, "[spans] %zu streams, %u scan points, %u spans\n", elig.size(), npts, nsp);
    if (nsp == (uint32_t)elig.size()) return 0;  // nothing to cut
    if (!room(h, h->sp_spans, sizeof(fl_span) * nsp) || !room(h, h->sp_res, sizeof(fl_span_res) * 2 * nsp) ||
        !room(h, h->sp_cand, sizeof(uint64_t) * (cand.size() + 1)) || !room(h, h->sp_candoff, sizeof(uint32_t) * (n_chunks + 1)) ||
        !room(h, h->sp_tails, (size_t)FP_TAIL * nsp) || !room(h, h->sp_tails_b, (size_t)FP_TAIL * nsp))
        return 0;
    if (hipMemcpyAsync(h->sp_spans.p, spans.data(), sizeof(fl_span) * nsp, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (!cand.empty() && hipMemcpyAsync(h->sp_cand.p, cand.data(), sizeof(uint64_t) * cand.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipMemcpyAsync(h->sp_candoff.p, cand_off.data(), sizeof(uint32_t) * (n_chunks + 1), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    // ---- the pool run A writes to (span_plan.h, fl_span_pool_pieces): it may take a quarter of what is free next to what
    // it holds already
    const uint64_t pieces = fl_span_pool_pieces(chunks.data(), elig, nsp, both);
    if (pieces * FP_PIECE > FL_SPAN_POOL_MAX) return 0;
    if (pieces * FP_PIECE + 16 > h->sp_pool.cap) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return 0;
        }
        if (pieces * FP_PIECE + 16 > h->sp_pool.cap + free_b / 4) return 0;
    }
    if (!room(h, h->sp_pool, (size_t)(pieces * FP_PIECE + 16)) || !room(h, h->sp_pooltab, sizeof(uint32_t) * (size_t)FP_MAX_PIECES * nsp * 2) ||
        !room(h, h->sp_poolctl, 16))
        return 0;
    if (hipMemsetAsync(h->sp_poolctl.p, 0, 16, st) != hipSuccess) return -1;
    const fl_span_pool pool = {(uint8_t*)h->sp_pool.p, /*next*/ (uint32_t*)h->sp_poolctl.p, /*tab*/ (uint32_t*)h->sp_pooltab.p, (uint32_t)pieces, /*pad*/ 0};
    // ---- run A
    {
        ProfScope ps(h, K_INFLATE_SPAN);
        hipLaunchKernelGGL(k_inflate_span, dim3(twin && !sym ? 2 * nsp : nsp), dim3(FP_THREADS), 0, st, d_in, dch, container, flags, h->crc, d_out,
                           (const fl_span*)h->sp_spans.p, (fl_span_res*)h->sp_res.p, (const uint64_t*)h->sp_cand.p,
                           (const uint32_t*)h->sp_candoff.p, (uint8_t*)h->sp_tails.p, 0u, pool, twin && !sym ? nsp : 0u,
                           (uint8_t*)h->sp_tails_b.p, sym ? nsp : 0u);
    }
    std::vector<fl_span_res> r1(nsp), r2(nsp);
    if (hipMemcpyAsync(r1.data(), h->sp_res.p, sizeof(fl_span_res) * nsp, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (twin && !sym && hipMemcpyAsync(r2.data(), (const fl_span_res*)h->sp_res.p + nsp, sizeof(fl_span_res) * nsp, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    if (sym) r2 = r1;  // (one decode: what it says holds for both planes)
    if (dbg) fprintf(stderr, "[spans] %.3f ms: sync 2 done\n", since());
    // ---- the chain of every stream
    std::vector<fl_span_chain> plans(elig.size());
    bool any = false;
    for (size_t k = 0; k < elig.size(); k++) {
        plans[k] = fl_span_follow_chain(spans.data(), r1.data(), sp_first[k], sp_first[k + 1], chunks[elig[k]].out_cap, both);
        if (dbg) span_debug_chain(plans[k], elig[k], spans, r1, sp_first[k], sp_first[k + 1]);
        any = any || plans[k].ok;
    }
    if (!any) return 0;
    // ---- run B with the other filling of the history (live spans, in place), the true tails, k_span_fix
    const fl_span_fix_plan fp = fl_span_fix_items(chunks.data(), elig, spans.data(), r1.data(), plans, nsp, both);
    const bool uses_hist = fp.uses_hist;
    if (dbg) fprintf(stderr, "[spans] history needed: %d\n", (int)uses_hist);
    const uint32_t n_items = (uint32_t)fp.items.size();
    if (!room(h, h->sp_chain, sizeof(uint32_t) * (fp.chain_all.size() + 1)) || !room(h, h->sp_chainoff, sizeof(uint32_t) * fp.chain_off.size()) ||
        !room(h, h->sp_items, sizeof(fl_fix_item) * ((size_t)n_items + 1)) || !room(h, h->sp_part, sizeof(uint32_t) * 2 * ((size_t)n_items + 1)))
        return 0;
    if (hipMemcpyAsync(h->sp_spans.p, spans.data(), sizeof(fl_span) * nsp, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipMemcpyAsync(h->sp_chain.p, fp.chain_all.data(), sizeof(uint32_t) * fp.chain_all.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    if (hipMemcpyAsync(h->sp_chainoff.p, fp.chain_off.data(), sizeof(uint32_t) * fp.chain_off.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    // (symbols) every span's place in its chain, room for two sets of tails in symbols; no room: span after span
    bool rs_ok = false;
    if (sym && uses_hist) {
        rs_ok = !fp.chain_pos.empty() && room(h, h->sp_chainpos, sizeof(uint32_t) * fp.chain_pos.size()) &&
                room(h, h->sp_rs, 2 * fp.chain_pos.size() * (size_t)FP_TAIL * sizeof(uint16_t));
        if (rs_ok && hipMemcpyAsync(h->sp_chainpos.p, fp.chain_pos.data(), sizeof(uint32_t) * fp.chain_pos.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    }
    if (n_items && hipMemcpyAsync(h->sp_items.p, fp.items.data(), sizeof(fl_fix_item) * n_items, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    {
        ProfScope ps(h, K_INFLATE_SPAN);
        if (uses_hist) {
            if (!both)
                hipLaunchKernelGGL(k_inflate_span, dim3(nsp), dim3(FP_THREADS), 0, st, d_in, dch, container, flags, h->crc, d_out,
                                   (const fl_span*)h->sp_spans.p, (fl_span_res*)h->sp_res.p, (const uint64_t*)h->sp_cand.p,
                                   (const uint32_t*)h->sp_candoff.p, (uint8_t*)h->sp_tails_b.p, 1u, pool, 0u, (uint8_t*)nullptr, 0u);
            if (sym && rs_ok) {
                // the true tails of all spans at once: log2(longest chain) steps (kernels_inflate_par.h, k_span_rs_*)
                const uint32_t ng = (uint32_t)fp.chain_all.size();
                uint16_t* S0 = (uint16_t*)h->sp_rs.p;
                uint16_t* S1 = S0 + (size_t)ng * FP_TAIL;
                const dim3 grid(ng, FP_TAIL / (256 * 8));
                hipLaunchKernelGGL(k_span_rs_init, grid, dim3(256), 0, st, (const uint32_t*)h->sp_chain.p, (const uint32_t*)h->sp_chainpos.p,
                                   (const uint8_t*)h->sp_tails.p, (const uint8_t*)h->sp_tails_b.p, S0);
                for (uint32_t D = 1; D < fp.longest; D *= 2) {
                    hipLaunchKernelGGL(k_span_rs_step, grid, dim3(256), 0, st, (const uint32_t*)h->sp_chainpos.p, (const uint16_t*)S0, S1, D);
                    std::swap(S0, S1);
                }
                hipLaunchKernelGGL(k_span_rs_out, grid, dim3(256), 0, st, (const uint32_t*)h->sp_chain.p, (const uint16_t*)S0, (uint8_t*)h->sp_tails.p);
            } else {
                hipLaunchKernelGGL(k_span_resolve, dim3((uint32_t)elig.size()), dim3(FP_THREADS), 0, st, (const uint32_t*)h->sp_chain.p,
                                   (const uint32_t*)h->sp_chainoff.p, (uint8_t*)h->sp_tails.p, (const uint8_t*)h->sp_tails_b.p);
            }
        }
        if (n_items)
            hipLaunchKernelGGL(k_span_fix, dim3(n_items / FP_FIX_WAVES), dim3(64 * FP_FIX_WAVES), 0, st, (const fl_fix_item*)h->sp_items.p, pool,
                               (const uint8_t*)h->sp_tails.p, d_out, container, h->crc, (uint32_t*)h->sp_part.p);
    }
    // the footers of the streams whose chain is whole (one small gather instead of a copy per stream)
    const uint32_t flen = fl_span_footer_len(container);
    const uint32_t nel = (uint32_t)elig.size();
    std::vector<uint64_t> foot_off(nel, ~0ull);
    std::vector<uint8_t> foot(8 * (size_t)nel, 0);
    if (flen) {
        for (uint32_t k = 0; k < nel; k++)
            if (const uint64_t at = fl_span_footer_at(plans[k], flen, chunks[elig[k]].in_len); at != ~0ull) foot_off[k] = chunks[elig[k]].in_off + at;
        if (!room(h, h->sp_footoff, sizeof(uint64_t) * nel) || !room(h, h->sp_foot, 8 * (size_t)nel)) return 0;
        if (hipMemcpyAsync(h->sp_footoff.p, foot_off.data(), sizeof(uint64_t) * nel, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_span_footers, dim3((nel + 63) / 64), dim3(64), 0, st, d_in, (const uint64_t*)h->sp_footoff.p, nel, flen,
                           (uint8_t*)h->sp_foot.p);
        if (hipMemcpyAsync(foot.data(), h->sp_foot.p, 8 * (size_t)nel, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    }
    std::vector<uint32_t> part(2 * (size_t)n_items);
    if (uses_hist && !both && hipMemcpyAsync(r2.data(), h->sp_res.p, sizeof(fl_span_res) * nsp, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (n_items && hipMemcpyAsync(part.data(), h->sp_part.p, sizeof(uint32_t) * 2 * n_items, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    if (dbg) fprintf(stderr, "[spans] %.3f ms: sync 3 done\n", since());
    // ---- run B as run A, the checksum, the footer
    const uint32_t pow_item = fl_crc_xpow8n(h->crc.xpow8, FP_FIX_ITEM);
    std::vector<fl_span_fin> fin;
    for (uint32_t k = 0; k < nel; k++) {
        const fl_span_chain& pl = plans[k];
        if (!pl.ok) continue;
        const fl_span_verdict v = fl_span_verify(pl, spans.data(), r1.data(), r2.data(), uses_hist, part.data() + 2 * (size_t)fp.item_first[k],
                                                 fp.item_first[k + 1] - fp.item_first[k], container, h->crc.xpow8, pow_item, &foot[8 * (size_t)k],
                                                 chunks[elig[k]].in_len);
        if (dbg && v.bad_b != ~0u) {
            const uint32_t si = pl.chain[v.bad_b];
            const fl_span_res &a = r1[si], &b = r2[si];
            fprintf(stderr, "[spans] span %u (chain %zu): run B status %u len %llu/%llu end %llu/%llu\n", si, (size_t)v.bad_b, b.status, (unsigned long long)b.out_len, (unsigned long long)a.out_len, (unsigned long long)b.end_bit, (unsigned long long)a.end_bit);
        }
        if (dbg) fprintf(stderr, "[spans] stream %u after k_span_fix: ok=%d crc %08x\n", elig[k], (int)v.ok, v.crc);
        if (!v.ok) continue;  // (the bytes written so far are written again by the kernels that follow)
        fin.push_back(fl_span_fin{pl.total, v.used, /*chunk*/ elig[k], /*pad*/ 0});
        chunks[elig[k]].skip = 1;
    }
    const int done = (int)fin.size();
    if (done) {
        if (!room(h, h->sp_fin, sizeof(fl_span_fin) * fin.size())) {
            for (const fl_span_fin& f : fin) chunks[f.chunk].skip = 0;  // (nobody wrote their results: the old way does)
            return 0;
        }
        if (hipMemcpyAsync(h->sp_fin.p, fin.data(), sizeof(fl_span_fin) * fin.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_span_finish, dim3(((uint32_t)fin.size() + 63) / 64), dim3(64), 0, st, (const fl_span_fin*)h->sp_fin.p,
                           (uint32_t)fin.size(), d_status, d_outlen, d_consumed);
        if (hipStreamSynchronize(st) != hipSuccess) return -1;  // (the source is on this stack)
    }
    if (dbg) fprintf(stderr, "[spans] %.3f ms: return\n", since());
    h->dbg_span_done = (uint64_t)done;
    return done;
}

// flate_hip_decompressed_sizes, long streams: cut each at block starts (k_span_scan, as try_span_inflate aims it but spaced
// by size_plan.h), count every span with a wave of its own and follow each stream's chain of span records on the host.
// A stream whose chain closes gets its size / status / consumed here and chunks[i].skip = 1; every other stream stays for
// the wave-per-stream launch.  Two host waits.  Returns the number of streams finished, or -1 (a HIP call failed).
// The long streams of a batch cut into spans and every span counted (k_inflate_size<true>): elig gets the streams that
// were looked at, spans / recs the spans of stream elig[k] at [sp_first[k], sp_first[k + 1]) with their records.  Returns
// the number of spans, 0 when nothing is cut, -1 when a HIP call fails.  The size probe follows the chains and sums; the
// index walk (index_walk) walks every span of a closed chain again for its points.
int size_span_records(flate_hip_ctx* h, hipStream_t st, const uint8_t* d_in, const std::vector<fl_chunk>& chunks, int container, int flags,
                      std::vector<uint32_t>& elig, std::vector<fl_size_span>& spans, std::vector<uint32_t>& sp_first,
                      std::vector<fl_size_rec>& recs) {
    const uint32_t n_chunks = (uint32_t)chunks.size();
    if (flags & 1) return 0;  // (as decompress: the scan's first two steps know the lenient header only)
    const uint32_t n_cu = device_cu_count(h);
    std::vector<uint64_t> lens(n_chunks);
    for (uint32_t i = 0; i < n_chunks; i++) lens[i] = chunks[i].skip ? 0 : chunks[i].in_len;
    std::vector<uint32_t> pieces;
    fl_size_eligible(lens.data(), n_chunks, h->knobs.span_min_bytes, n_cu, elig);
    if (elig.empty()) return 0;
    std::vector<uint64_t> elens(elig.size());
    for (size_t k = 0; k < elig.size(); k++) elens[k] = lens[elig[k]];
    fl_size_spacing(elens.data(), (uint32_t)elig.size(), n_cu, pieces);
    // ---- where spans may start
    std::vector<fl_scan_point> points;
    std::vector<uint32_t> pt_first(elig.size() + 1, 0);
    std::vector<uint64_t> fl;
    for (size_t k = 0; k < elig.size(); k++) {
        fl.clear();
        fl_size_targets(elens[k], pieces[k], fl);
        for (size_t j = 0; j + 1 < fl.size(); j += 2) {
            fl_scan_point pt;
            pt.from_bit = fl[j];
            pt.limit_bit = fl[j + 1];
            pt.stream = elig[k];
            pt.pad = 0;
            points.push_back(pt);
        }
        pt_first[k + 1] = (uint32_t)points.size();
    }
    const uint32_t npts = (uint32_t)points.size();
    if (!npts) return 0;
    std::vector<uint64_t> found;
    if (const int sc = scan_block_starts(h, st, d_in, flags, points, found); sc <= 0) return sc;
    const fl_chunk* dch = (const fl_chunk*)h->chunks.p;
    // ---- the spans: the stream start, then every distinct position found; a span ends where the next one starts
    spans.clear();
    sp_first.assign(elig.size() + 1, 0);
    for (size_t k = 0; k < elig.size(); k++) {
        fl_size_span s0;
        s0.start_bit = 0;
        s0.stop_bit = ~0ull;
        s0.stream = elig[k];
        s0.first = 1;
        spans.push_back(s0);
        s0.first = 0;
        for (uint64_t p : fl_cut_positions(found.data(), pt_first[k], pt_first[k + 1], elens[k] * 8)) {
            spans.back().stop_bit = p;
            s0.start_bit = p;
            spans.push_back(s0);
        }
        sp_first[k + 1] = (uint32_t)spans.size();
    }
    const uint32_t nsp = (uint32_t)spans.size();
    if (nsp == (uint32_t)elig.size()) return 0;  // nothing to cut
    if (!room(h, h->sz_spans, sizeof(fl_size_span) * nsp) || !room(h, h->sz_recs, sizeof(fl_size_rec) * nsp)) return 0;
    if (hipMemcpyAsync(h->sz_spans.p, spans.data(), sizeof(fl_size_span) * nsp, hipMemcpyHostToDevice, st) != hipSuccess) return -1;
    {
        ProfScope ps(h, K_INFLATE_SIZE_SPAN);
        hipLaunchKernelGGL(k_inflate_size<true>, dim3(nsp), dim3(64), 0, st, d_in, dch, container, flags, (uint64_t*)nullptr,
                           (int32_t*)nullptr, (uint64_t*)nullptr, (const fl_size_span*)h->sz_spans.p, (fl_size_rec*)h->sz_recs.p);
    }
    recs.resize(nsp);
    if (hipMemcpyAsync(recs.data(), h->sz_recs.p, sizeof(fl_size_rec) * nsp, hipMemcpyDeviceToHost, st) != hipSuccess) return -1;
    if (hipStreamSynchronize(st) != hipSuccess) return -1;
    return (int)nsp;
}

// what size_span_records found, kept by a caller that walks the same streams behind the probe (flate_hip_index_scan)
struct SpanRecords {
    std::vector<uint32_t> elig, sp_first;
    std::vector<fl_size_span> spans;
    std::vector<fl_size_rec> recs;
    int nsp = 0;
};

int size_by_spans(flate_hip_ctx* h, hipStream_t st, const uint8_t* d_in, std::vector<fl_chunk>& chunks, int container, int flags,
                  uint64_t* d_sizes, int32_t* d_status, uint64_t* d_consumed, SpanRecords* keep = nullptr) {
    SpanRecords own;
    SpanRecords& sr = keep ? *keep : own;
    std::vector<uint32_t>&elig = sr.elig, &sp_first = sr.sp_first;
    std::vector<fl_size_span>& spans = sr.spans;
    std::vector<fl_size_rec>& recs = sr.recs;
    sr.nsp = size_span_records(h, st, d_in, chunks, container, flags, elig, spans, sp_first, recs);
    if (sr.nsp <= 0) return sr.nsp;
    // ---- the chains
    std::vector<fl_span_fin> fin;
    for (size_t k = 0; k < elig.size(); k++) {
        const uint32_t a = sp_first[k], b = sp_first[k + 1];
        if (b - a < 2) continue;  // not cut: the whole-stream launch counts it
        uint64_t size = 0, used = 0;
        int32_t stt = 0;
        if (!fl_size_follow_chain(spans.data() + a, recs.data() + a, b - a, &size, &stt, &used)) continue;
        fin.push_back(fl_span_fin{size, used, /*chunk*/ elig[k], /*pad*/ 0});
        chunks[elig[k]].skip = 1;
    }
    if (!fin.empty()) {
        if (!room(h, h->sp_fin, sizeof(fl_span_fin) * fin.size())) {
            for (const fl_span_fin& f : fin) chunks[f.chunk].skip = 0;
            return 0;
        }
        if (hipMemcpyAsync(h->sp_fin.p, fin.data(), sizeof(fl_span_fin) * fin.size(), hipMemcpyHostToDevice, st) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_span_finish, dim3(((uint32_t)fin.size() + 63) / 64), dim3(64), 0, st, (const fl_span_fin*)h->sp_fin.p,
                           (uint32_t)fin.size(), d_status, d_sizes, d_consumed);
        if (hipStreamSynchronize(st) != hipSuccess) return -1;  // (the source is on this stack)
    }
    return (int)fin.size();
}

}  // namespace

extern "C" {

const char* flate_hip_version(void) { return "flate_hip 0.1 (gfx950)"; }

const char* flate_hip_status_name(int s) {
    switch (s) {
        case 0: return "Ok";
        case 1: return "EndOfStream";
        case 2: return "BadGzipHeader";
        case 3: return "BadZlibHeader";
        case 4: return "WrongGzipChecksum";
        case 5: return "WrongGzipSize";
        case 6: return "WrongZlibChecksum";
        case 7: return "InvalidCode";
        case 8: return "OversubscribedHuffmanTree";
        case 9: return "IncompleteHuffmanTree";
        case 10: return "MissingEndOfBlockCode";
        case 11: return "InvalidMatch";
        case 12: return "InvalidBlockType";
        case 13: return "WrongStoredBlockNlen";
        case 14: return "InvalidDynamicBlockHeader";
        case 100: return "OutputTooSmall";
        case 101: return "ChunkTooLarge";
        case 102: return "ReferenceQ1Stream";
        case 104: return "NeedInput";
        case 105: return "NeedOutput";
        case 106: return "NeedDict";
        case 107: return "WrongDict";
        default: return "Unknown";
    }
}

int flate_hip_create(int device, flate_hip_handle* out) {
    if (!out) return FLATE_HIP_E_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return FLATE_HIP_E_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    flate_hip_ctx* h = new flate_hip_ctx();
    h->device = device;
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return FLATE_HIP_E_NO_DEVICE;
    }
    h->stream = h->own_stream;
    init_crc_consts(h->crc);
    read_knobs(h->knobs, FL_SPAN_MIN_BYTES);
    *out = h;
    return FLATE_HIP_OK;
}

// Debug / test seam: read the FLATE_HIP_* tuning variables again (they are read once, when the handle is made).
int flate_hip_debug_reload_env(flate_hip_handle h) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    read_knobs(h->knobs, FL_SPAN_MIN_BYTES);
    return FLATE_HIP_OK;
}

int flate_hip_destroy(flate_hip_handle h) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    fold_profile(h);
    for (PinBuf* b : {&h->pin_in, &h->pin_len, &h->pin_tab, &h->pin_out}) pin_release(*b);
    for (DevBuf* b : {&h->sp_points, &h->sp_found, &h->sp_spans, &h->sp_res, &h->sp_cand, &h->sp_candoff, &h->sp_tails,
                      &h->sp_tails_b, &h->sp_chain, &h->sp_chainoff, &h->sp_pool, &h->sp_pooltab, &h->sp_poolctl, &h->sp_items,
                      &h->sp_part, &h->sp_footoff, &h->sp_foot, &h->sp_fin, &h->sp_chainpos, &h->sp_rs, &h->sz_spans, &h->sz_recs})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf* b : {&h->mb_tiles, &h->mb_tileoff, &h->mb_cand, &h->mb_chunks, &h->mb_psize, &h->mb_pstatus, &h->mb_pcons,
                      &h->mb_succ, &h->mb_chain, &h->mb_taboff, &h->mb_tabn, &h->mb_non, &h->mb_tabstart, &h->mb_tabsize,
                      &h->mb_denseoff, &h->mb_dstart, &h->mb_dsize, &h->mb_outlen, &h->mb_status, &h->mb_cons, &h->mb_nmem})
        if (b->p) (void)hipFree(b->p);
    for (DevBuf* b : {&h->chunks, &h->blk_chunk, &h->plans, &h->hist, &h->cks, &h->S, &h->NC, &h->rec, &h->desc, &h->marks,
                      &h->tokens, &h->ntok, &h->cflag, &h->links, &h->wchunks, &h->swins, &h->wexit, &h->shard_sz, &h->tiles, &h->segs, &h->pieces, &h->fpts, &h->zones, &h->nsorted, &h->jmp,
                      &h->exitmap, &h->entry, &h->segtok, &h->tokbase, &h->bound, &h->sgroups, &h->sgroup0, &h->gmap, &h->gentry,
                      &h->sblocks, &h->st_in, &h->st_out, &h->st_inoff, &h->st_outlen, &h->st_status,
                      &h->st_consumed, &h->st_pack, &h->st_packoff, &h->st_slot, &h->dbg_par_handed, &h->dc_tab, &h->dc_bytes, &h->dc_of, &h->dcc_stage,
                      &h->dcc_jobs, &h->dcc_chunks, &h->jn_scratch, &h->jn_streams, &h->jn_pstream, &h->jn_slot, &h->jn_len,
                      &h->jn_status, &h->jn_cks, &h->jn_dst, &h->jn_scks, &h->ix_jobs, &h->ix_recs, &h->ix_ptbit, &h->ix_ptpos, &h->ix_wtab,
                      &h->ix_rjobs, &h->ix_rtab, &h->ix_scratch, &h->jn_which, &h->jn_place, &h->ix_pjobs, &h->ix_ptab, &h->ix_plen,
                      &h->ix_pstatus, &h->ix_rrec, &h->ix_rdst, &h->ix_entries, &h->ix_epack})
        if (b->p) (void)hipFree(b->p);
    h->ws_bytes = 0;  // (every buffer ensure() grew is one of the above)
    for (hipEvent_t e : h->free_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->xfer_events) (void)hipEventDestroy(e);
    if (h->c2_ev0) (void)hipEventDestroy(h->c2_ev0);
    if (h->c2_ev1) (void)hipEventDestroy(h->c2_ev1);
    if (h->s_c2) (void)hipStreamDestroy(h->s_c2);
    if (h->ms_ev0) (void)hipEventDestroy(h->ms_ev0);
    if (h->ms_ev1) (void)hipEventDestroy(h->ms_ev1);
    if (h->s_ms) (void)hipStreamDestroy(h->s_ms);
    if (h->ck_ev0) (void)hipEventDestroy(h->ck_ev0);
    if (h->ck_ev1) (void)hipEventDestroy(h->ck_ev1);
    if (h->s_ck) (void)hipStreamDestroy(h->s_ck);
    if (h->s_in) (void)hipStreamDestroy(h->s_in);
    if (h->s_out) (void)hipStreamDestroy(h->s_out);
    (void)hipStreamDestroy(h->own_stream);
    delete h;
    return FLATE_HIP_OK;
}

int flate_hip_set_stream(flate_hip_handle h, void* hip_stream) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    hipStream_t next = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    if (next != h->stream) {
        // work enqueued on the old stream still uses the workspace: drain it before the next call
        // (which may grow, i.e. free, those buffers) runs on another stream
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        fold_profile(h);
    }
    h->stream = next;
    return FLATE_HIP_OK;
}
int flate_hip_set_sync(flate_hip_handle h, int s) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    h->sync = s != 0;
    return FLATE_HIP_OK;
}
const char* flate_hip_last_error(flate_hip_handle h) { return h ? h->last_error.c_str() : "null handle"; }

size_t flate_hip_compress_bound(size_t n, int container, int mode) {
    (void)mode;
    const size_t hdr = container == 1 ? 18 : (container == 2 ? 6 : 0);
    // stored blocks: 5 bytes per 65535 (+ a possibly empty trailing one); a Huffman block never
    // beats that bound by more than its header; slack for the Q1 seam.
    return (size_t)fl_raw_bound(n) + hdr;
}

size_t flate_hip_joined_bound(uint64_t n, uint32_t piece_bytes, int container, int mode) {
    (void)mode;
    return (size_t)fl_join_bound(n, fl_join_piece_bytes(piece_bytes > FL_JOIN_MAX_PIECE ? 0u : piece_bytes), container);
}

int flate_hip_profile_enable(flate_hip_handle h, int enable) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    h->prof = enable != 0;
    return FLATE_HIP_OK;
}
int flate_hip_profile_reset(flate_hip_handle h) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    fold_profile(h);
    for (int i = 0; i < K_COUNT; i++) {
        h->prof_ms[i] = 0;
        h->prof_n[i] = 0;
    }
    return FLATE_HIP_OK;
}
int flate_hip_profile_read(flate_hip_handle h, const char** names, double* total_ms, uint64_t* launches, int cap) {
    if (!h) return FLATE_HIP_E_INVALID_ARG;
    fold_profile(h);
    int n = 0;
    for (int i = 0; i < K_COUNT && n < cap; i++) {
        if (!h->prof_n[i]) continue;
        names[n] = kKernelNames[i];
        total_ms[n] = h->prof_ms[i];
        launches[n] = h->prof_n[i];
        n++;
    }
    return n;
}

}  // extern "C"

namespace {
// ---- compress_impl: every compress entry point.  Its decisions are pass_plan.h's (plain C++, tested on the CPU); the
// functions below carry them out, one per stage, over one record per call.

// Pageable callers' buffers behind pinned mirrors (run_on_mirrors): a sub-batch's input is copied into the mirror right
// before its H2D copy is enqueued, its produced bytes out of the mirror as soon as they have landed -- while the GPU works
// on the other sub-batches.  State of ONE call: the call that runs on the mirrors is handed a pointer to it.
struct Mirror {
    const uint8_t* src = nullptr;   // the caller's input from in_lo on, and its mirror
    uint8_t* pin = nullptr;
    const uint8_t* pout = nullptr;  // the output's mirror from out_lo on, and the caller's output
    uint8_t* out = nullptr;
    const uint64_t* out_len = nullptr;
    const uint64_t *hin = nullptr, *hout = nullptr;
    uint64_t in_lo = 0, out_lo = 0;
    unsigned nt = 1;  // host threads that copy
    bool landed = false;
    template <class F>
    void parallel(uint64_t items, const F& fn) const {
        std::vector<std::thread> th;
        const uint64_t per = (items + nt - 1) / nt;
        for (unsigned t = 1; t < nt; t++) {
            const uint64_t a = std::min(items, t * per), b = std::min(items, a + per);
            if (b > a) th.emplace_back(fn, a, b);
        }
        fn(0, std::min(items, per));
        for (auto& x : th) x.join();
    }
    void copy_in(uint32_t c0, uint32_t nc) const {
        const uint64_t a = hin[c0] - in_lo, b = hin[c0 + nc] - in_lo;
        parallel(b - a, [&](uint64_t x, uint64_t y) { memcpy(pin + a + x, src + a + x, y - x); });
    }
    void copy_out(uint32_t c0, uint32_t nc) {
        landed = true;
        parallel(nc, [&](uint64_t x, uint64_t y) {
            for (uint64_t i = c0 + x; i < c0 + y; i++) {
                const uint64_t n = std::min<uint64_t>(out_len[i], hout[i + 1] - hout[i]);
                if (n) memcpy(out + hout[i], pout + (hout[i] - out_lo), n);
            }
        });
    }
};

// The dictionaries of a flate_hip_compress_batch_dict call, as compress_impl is handed them: the offsets are on the host
// already, the dictionaries' bytes and their table (Adler-32s filled) on the device.
struct DictCall {
    std::vector<uint64_t> hin, hout;
    std::vector<fl_dictc_stream> streams;  // one per chunk
    const uint8_t* d_dict = nullptr;
    const fl_dict_ent* d_tab = nullptr;
};

// What the stages of one compress_impl call share.
struct CompressCall {
    flate_hip_ctx* h = nullptr;
    // the caller's arguments
    const uint8_t* in = nullptr;
    uint8_t* out = nullptr;
    uint64_t* out_len = nullptr;
    int32_t* status = nullptr;
    uint32_t n_chunks = 0;
    int container = 0, mode = 0, memkind = 0;
    const FlushSpec* fs = nullptr;
    const DictCall* dc = nullptr;  // flate_hip_compress_batch_dict: streams with preset dictionaries (never mirrored, pinned or planned)
    // pl: the batch's layout is known (plan): no offsets are fetched; while the plan is being built
    // (!pl->ready, `planning`) the per-pass tables are made and kept and nothing is launched, afterwards
    // (`planned_run`) they are used as they are and the call only enqueues work
    flate_hip_plan* pl = nullptr;
    bool planning = false, planned_run = false;
    Mirror* mirror = nullptr;  // the call runs on a pageable caller's mirrors
    hipStream_t st = nullptr;  // the caller's stream
    fl_params prm{};
    std::vector<uint64_t> hin_, hout_;  // the offsets on the host (a plan holds its own)
    const std::vector<uint64_t>*hin = nullptr, *hout = nullptr;
    uint64_t in_lo = 0, in_hi = 0, out_lo = 0, out_hi = 0;
    // device views of the caller's buffers
    const uint8_t* d_in = nullptr;
    uint8_t* d_out = nullptr;
    uint64_t* d_outlen = nullptr;
    int32_t* d_status = nullptr;
    uint64_t in_shift = 0, out_shift = 0;  // subtracted from offsets when staging host buffers
    bool pin_in = false, pin_out = false;
    bool pinned_passes = false;  // the tables of a pass travel on the input stream (prepare_pinned_tables)
    bool landing = false;        // a mirrored call whose passes' output leaves the mirror as it lands
    uint8_t* zc_out = nullptr;   // device view of out + out_lo
    std::vector<uint64_t> zc_slot;
    // the tables: the copies of the pinned path read them until the call ends (PassGuard)
    std::vector<fl_chunk> chunks;
    std::deque<std::vector<uint32_t>> keep_blk;
    std::deque<std::vector<fl_sblock>> keep_sb;
    std::vector<uint32_t> pass_c0;  // first chunk of every pass (Mirror::copy_out)
    uint64_t blk_total = 0, blk_base = 0;  // pinned path: block slots of the whole batch, and those of the passes so far
    fl_pass_cfg pcfg;
    bool two = false;      // the passes alternate between two compute streams
    fl_two_slices slices;  // ... over these slices of the workspace
};

// One pass [c0, c0 + nc) on its way through the stages
struct PassRun {
    uint32_t c0 = 0, nc = 0, nb = 0;
    size_t index = 0;
    bool stream = false;           // a whole-stream pass
    bool staged = false;           // ... of streams with preset dictionaries: its kernels read the staging workspace
    std::vector<fl_dictc_job> jobs;    // ... the staging kernel's table
    std::vector<fl_chunk> rec_chunks;  // ... and the chunk table of the records alone (the checksum covers no dictionary)
    bool sliced = false;           // this pass's tables: a slice of their own, filled on the input stream
    hipEvent_t ev_in = nullptr;    // its input (and tables) are on the device
    hipStream_t stp = nullptr;     // the compute stream its kernels run on
    const fl_chunk* dch = nullptr; // its tables on the device
    const uint32_t* dbc = nullptr;
    const fl_sblock* dsb = nullptr;
    StreamTables tabs;
    std::vector<uint32_t>* blk_chunk = nullptr;
    std::vector<fl_sblock>* sblocks = nullptr;  // huffman-only / store-only with flush points
};

struct MsGuard {  // (whatever way this call ends, the caller's stream is behind the clearing)
    flate_hip_ctx* h;
    ~MsGuard() {
        if (h->ms_pending) {
            (void)hipStreamWaitEvent(h->stream, h->ms_ev1, 0);
            h->ms_pending = false;
        }
    }
};
// On the pinned path the passes are enqueued without a host wait in between and the copies on the input stream read the
// call's vectors: whichever way compress_impl is left (an error in the middle included), they are outlived by the copies,
// and on two compute streams no kernel of the second one still writes the caller's output.
struct PassGuard {
    flate_hip_ctx* h;
    bool on;
    ~PassGuard() {
        if (on) {
            if (h->s_in) (void)hipStreamSynchronize(h->s_in);
            if (h->s_c2) (void)hipStreamSynchronize(h->s_c2);
            (void)hipStreamSynchronize(h->stream);
        }
        h->ck_pending = false;  // (an error between the checksum launch and the back end must not leave a stale wait)
    }
};
struct WsFixed {
    flate_hip_ctx* h;
    ~WsFixed() { h->ws_fixed = false; }
};
struct WsShift {  // a pass's view of the two-slice workspace: every buffer from its slice on (undone when the pass is enqueued)
    std::vector<std::pair<DevBuf*, size_t>> undo;
    void add(DevBuf& b, size_t bytes) {
        b.p = (uint8_t*)b.p + bytes;
        b.cap -= bytes;
        undo.emplace_back(&b, bytes);
    }
    ~WsShift() {
        for (auto& u : undo) {
            u.first->p = (uint8_t*)u.first->p - u.second;
            u.first->cap += u.second;
        }
    }
};

int compress_impl(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks, int container,
                  int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, int memkind,
                  const FlushSpec* fs, flate_hip_plan* pl = nullptr, Mirror* mirror = nullptr, const DictCall* dc = nullptr,
                  const JoinCall* jc = nullptr);

// Pageable host buffers of some size (what every caller of the facade's compress(reader, writer) has): a
// staged hipMemcpy each way moves about 10 GB/s and nothing overlaps.  Instead a few host threads copy the
// input into a pinned mirror, the call runs on the mirrors (sub-batches, DMA copies on their own streams
// beside the kernels: the pinned path), and the threads copy the produced bytes out of the mirror.
// (Pinned buffers are used where they lie: no host thread touches the data.  On a shared host both ways have their
// bad minutes -- the direct one 16.6 instead of 10.1 ms in one process of five, the mirrors 17.6 instead of 11.3 when
// the neighbours keep the memory system busy -- and the direct one needs no CPU.)
// *taken: the call went this way and is over.
int run_on_mirrors(CompressCall& cc, const uint64_t* in_off, const uint64_t* out_off, bool* taken) {
    flate_hip_ctx* h = cc.h;
    *taken = false;
    if (!(cc.memkind == FLATE_HIP_MEM_HOST && !cc.fs && !cc.dc && !cc.pl && (cc.in_hi - cc.in_lo) >= (8ull << 20) && cc.in && cc.out && !cc.mirror &&
          !is_pinned_host(cc.in + cc.in_lo) && !is_pinned_host(cc.out + cc.out_lo) && !h->knobs.no_pin_mirror))
        return FLATE_HIP_OK;
    const size_t want_in = (cc.in_hi - cc.in_lo) + 16, want_out = (cc.out_hi - cc.out_lo) + 16;
    if (!pin_grow(h->pin_in, want_in, want_in + want_in / 8 + 4096) || !pin_grow(h->pin_out, want_out, want_out + want_out / 8 + 4096))
        return FLATE_HIP_OK;
    *taken = true;
    // the mirrors take the place of the caller's buffers: same offsets.  A sub-batch's input is copied right before
    // its H2D copy is enqueued, its produced bytes leave the mirror as soon as they have landed.
    Mirror m;
    m.src = cc.in + cc.in_lo;
    m.pin = (uint8_t*)h->pin_in.p;
    m.pout = (const uint8_t*)h->pin_out.p;
    m.out = cc.out;
    m.out_len = cc.out_len;
    m.hin = cc.hin->data();
    m.hout = cc.hout->data();
    m.in_lo = cc.in_lo;
    m.out_lo = cc.out_lo;
    m.nt = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    const int rc = compress_impl(h, m.pin - cc.in_lo, in_off, cc.n_chunks, cc.container, cc.mode, (uint8_t*)h->pin_out.p - cc.out_lo,
                                 out_off, cc.out_len, cc.status, cc.memkind, nullptr, nullptr, &m);
    if (rc) return rc;
    if (!m.landed) m.copy_out(0, cc.n_chunks);  // (the call did not take the overlapped path)
    // (large mirrors do not stay pinned with the handle)
    if (h->pin_in.cap > (1ull << 30)) pin_release(h->pin_in);
    if (h->pin_out.cap > (1ull << 30)) pin_release(h->pin_out);
    return FLATE_HIP_OK;
}

// Host buffers are staged: the device views, the shifts, and whether the copies run as DMA on streams of their own
int stage_host_buffers(CompressCall& cc) {
    flate_hip_ctx* h = cc.h;
    int rc;
    cc.d_in = cc.in;
    cc.d_out = cc.out;
    cc.d_outlen = cc.out_len;
    cc.d_status = cc.status;
    if (cc.memkind == FLATE_HIP_MEM_HOST) {
        if ((rc = ensure(h, h->st_in, (cc.in_hi - cc.in_lo) + 16))) return rc;
        if ((rc = ensure(h, h->st_out, (cc.out_hi - cc.out_lo) + 16))) return rc;
        if ((rc = ensure(h, h->st_outlen, sizeof(uint64_t) * cc.n_chunks))) return rc;
        if ((rc = ensure(h, h->st_status, sizeof(int32_t) * cc.n_chunks))) return rc;
        // Pinned host buffers (hipHostMalloc / hipHostRegister, torch pin_memory): the copies are real DMA
        // and run on their own streams, a sub-batch at a time (below).  Pageable: one staged copy each way.
        cc.pin_in = !cc.fs && !cc.dc && is_pinned_host(cc.in + cc.in_lo);
        cc.pin_out = !cc.fs && !cc.dc && is_pinned_host(cc.out + cc.out_lo);
        if ((cc.pin_in && !h->s_in && create_copy_stream(&h->s_in, true) != hipSuccess) ||
            (cc.pin_out && !h->s_out && create_copy_stream(&h->s_out, false) != hipSuccess))
            return FLATE_HIP_E_ALLOC;
        if (cc.in_hi > cc.in_lo && !cc.pin_in)
            HIP_OK(h, hipMemcpyAsync(h->st_in.p, cc.in + cc.in_lo, cc.in_hi - cc.in_lo, hipMemcpyHostToDevice, cc.st));
        cc.d_in = (const uint8_t*)h->st_in.p;
        cc.d_out = (uint8_t*)h->st_out.p;
        cc.d_outlen = (uint64_t*)h->st_outlen.p;
        cc.d_status = (int32_t*)h->st_status.p;
        cc.in_shift = cc.in_lo;
        cc.out_shift = cc.out_lo;
    } else if (((uintptr_t)cc.out & 3) != 0) {
        return FLATE_HIP_E_INVALID_ARG;
    }
    return FLATE_HIP_OK;
}

// the bit packer ORs into the output: clear the slots first -- on a stream of its own, behind what the caller's stream holds
// so far; the back end's first kernel that writes the slots waits for it (enqueue_back_end).  The tokenizer / the histograms
// and the planner do not touch the slots: 0.08 ms of config #4's 0.98 and 0.15 ms of the headline's 26.5 are hidden.
// (MsGuard puts the caller's stream behind the clearing when the call ends)
int clear_slots(CompressCall& cc) {
    flate_hip_ctx* h = cc.h;
    if (!(cc.out_hi > cc.out_lo && !cc.planning)) return FLATE_HIP_OK;
    if (!h->s_ms) (void)side_stream(h->s_ms, h->ms_ev0, h->ms_ev1);
    if (h->s_ms && !h->knobs.memset_inline) {
        HIP_OK(h, hipEventRecord(h->ms_ev0, cc.st));
        HIP_OK(h, hipStreamWaitEvent(h->s_ms, h->ms_ev0, 0));
        {
            ProfScope ps(h, K_MEMSET, h->s_ms);
            HIP_OK(h, hipMemsetAsync(cc.d_out + (cc.out_lo - cc.out_shift), 0, cc.out_hi - cc.out_lo, h->s_ms));
        }
        HIP_OK(h, hipEventRecord(h->ms_ev1, h->s_ms));
        h->ms_pending = true;
    } else {
        ProfScope ps(h, K_MEMSET);
        HIP_OK(h, hipMemsetAsync(cc.d_out + (cc.out_lo - cc.out_shift), 0, cc.out_hi - cc.out_lo, cc.st));
    }
    return FLATE_HIP_OK;
}

// Pinned output: the link is shared by both directions (57 GB/s one way, 28.6 each way at once: tools/pcie_probe.py),
// so what must not cross it is the unused part of the slots.  A copy kernel on the output stream writes the
// produced bytes of every slot straight into the caller's (device-visible) pinned memory: 52 GB/s for the bytes
// that matter (tools/zero_copy_probe.py) instead of 57 GB/s for 2.5 x as many.  Bytes of a slot beyond out_len[i]
// are then not touched at all.
// Pinned path: the tables of a pass (chunk table, block -> chunk) are copies from pageable vectors, which the runtime
// stages and moves with a blit kernel -- 0.3-0.4 ms each time, on the compute stream between two passes (rocprofv3
// timeline, tools/e2e_timeline.py).  They go on the input stream instead, into a slice of their own per pass, ahead of
// the pass's input; the compute stream waits for one event per pass.
int prepare_pinned_tables(CompressCall& cc) {
    flate_hip_ctx* h = cc.h;
    int rc;
    const uint32_t n_chunks = cc.n_chunks;
    if (cc.pin_out) HIP_OK(h, hipStreamSynchronize(h->s_out));  // (nothing of an earlier call may still read st_out)
    if (cc.pin_out && cc.out_hi > cc.out_lo) {
        void* dp = nullptr;
        if (hipHostGetDevicePointer(&dp, cc.out + cc.out_lo, 0) == hipSuccess && dp) {
            cc.zc_out = (uint8_t*)dp;
            cc.zc_slot.resize((size_t)n_chunks + 1);
            for (uint32_t i = 0; i <= n_chunks; i++) cc.zc_slot[i] = (*cc.hout)[i] - cc.out_lo;
            if ((rc = ensure(h, h->st_slot, sizeof(uint64_t) * ((size_t)n_chunks + 1)))) return rc;
            HIP_OK(h, hipMemcpyAsync(h->st_slot.p, cc.zc_slot.data(), sizeof(uint64_t) * ((size_t)n_chunks + 1), hipMemcpyHostToDevice, cc.st));
        } else {
            (void)hipGetLastError();
        }
    }
    cc.pinned_passes = (cc.pin_in || cc.pin_out) && !cc.pl;
    if (cc.pinned_passes) {
        if (!h->s_in && create_copy_stream(&h->s_in, true) != hipSuccess) return FLATE_HIP_E_ALLOC;
        cc.blk_total = fl_batch_blocks(cc.chunks.data(), n_chunks, cc.mode);
        if ((rc = ensure(h, h->chunks, sizeof(fl_chunk) * (size_t)n_chunks))) return rc;
        if ((rc = ensure(h, h->blk_chunk, sizeof(uint32_t) * (size_t)std::max<uint64_t>(cc.blk_total, 1)))) return rc;
        HIP_OK(h, hipStreamSynchronize(h->s_in));  // (nothing of an earlier call may still write the tables)
        // the tables leave from pinned memory: [fl_chunk x n_chunks | uint32 x blk_total]
        const size_t tab_need = sizeof(fl_chunk) * (size_t)n_chunks + sizeof(uint32_t) * (size_t)std::max<uint64_t>(cc.blk_total, 1);
        if (!pin_grow(h->pin_tab, tab_need, tab_need + tab_need / 4 + 4096)) return FLATE_HIP_E_ALLOC;
    }
    return FLATE_HIP_OK;
}

int size_two_slices(flate_hip_ctx* h, const fl_params& prm, uint64_t nc, uint64_t nb) {
    int r;
    if ((r = ensure_lz_workspace(h, (uint32_t)(2 * nc), prm.chain))) return r;
    return ensure_block_workspace(h, 2 * nb);
}

// Two compute streams (pass_plan.h, fl_two_eligible: when, and why) and their workspace (fl_two_slices).  The other streams
// that touch a slice:
// - s_ck (k_checksum of containers 1 and 2 at levels 4..7, launch_checksum_side) writes the pass's `cks` slice behind an
//   event recorded on the pass's stream after the pass's own k_lz_chain -- after pass k's back end, which reads that slice;
// - s_in writes the batch-wide tables and input only (a slice of their own per pass), never the workspace.
// Everything is sized HERE, before the first pass is enqueued: ensure() synchronises only h->stream, which enqueue_sliced
// swaps, and would free a buffer the other stream still uses.  Until every pass is enqueued ensure() refuses to grow a
// buffer (h->ws_fixed): enqueue_pass's ensure_lz_workspace on the slice is a check, never a reallocation of a shifted buffer.
// Slices that cannot be had: the passes one after the other on the caller's stream (round 5's way).
void setup_two_streams(CompressCall& cc) {
    flate_hip_ctx* h = cc.h;
    cc.two = fl_two_eligible(cc.pcfg, cc.pinned_passes, cc.planned_run ? cc.pl->passes.size() : 0, cc.mode, cc.fs != nullptr || cc.dc != nullptr,
                             h->knobs.one_stream, cc.chunks.data());
    if (cc.two && !h->s_c2) cc.two = side_stream(h->s_c2, h->c2_ev0, h->c2_ev1);
    if (!cc.two) return;
    cc.two = cc.planned_run ? fl_two_from_plan(cc.pl->passes, cc.slices) : fl_two_from_schedule(cc.pcfg, cc.slices);
    if (cc.two && size_two_slices(h, cc.prm, cc.slices.nc, cc.slices.nb)) {
        (void)hipGetLastError();
        cc.two = false;
    }
}

// a pass over slice k & 1 of every per-pass buffer, its kernels on that stream
int enqueue_sliced(CompressCall& cc, size_t k, uint32_t nc, uint32_t nb, uint32_t c0, const fl_chunk* dch, const uint32_t* dbc,
                   const fl_sblock* dsb) {
    flate_hip_ctx* h = cc.h;
    const std::vector<fl_pass>& sched = cc.slices.sched;
    if (k >= sched.size() || sched[k].c0 != c0 || sched[k].nc != nc || nc > cc.slices.nc || nb > cc.slices.nb) {
        h->last_error = "two-stream pass " + std::to_string(k) + " (" + std::to_string(c0) + " + " + std::to_string(nc) +
                        " chunks) is not the scheduled one";
        return FLATE_HIP_E_LAUNCH;
    }
    const uint32_t slice = sched[k].stream;
    hipStream_t sq = slice ? h->s_c2 : cc.st;
    WsShift ws;
    const size_t c_sl = (size_t)slice * cc.slices.nc, b0 = (size_t)slice * cc.slices.nb;
    const bool bulk = cc.prm.chain >= FL_BULK_MIN_CHAIN;
    const fl_lz_sizes z = fl_lz_chunk_sizes(bulk);
    const fl_blk_sizes bs = fl_block_slot_sizes();
    ws.add(h->plans, bs.plan * b0);
    ws.add(h->hist, bs.hist * b0);
    ws.add(h->cks, bs.cks * b0);
    ws.add(bulk ? h->links : h->S, z.links * c_sl);
    ws.add(h->desc, z.desc * c_sl);
    ws.add(h->marks, z.marks * c_sl);
    ws.add(h->tokens, z.tokens * c_sl);
    ws.add(h->ntok, z.ntok * c_sl);
    ws.add(h->cflag, z.cflag * c_sl);
    hipStream_t saved = h->stream;
    h->stream = sq;
    const int r = enqueue_pass(h, cc.prm, nc, nb, c0, dch, dbc, dsb, cc.d_in, cc.d_out, cc.d_outlen, cc.d_status);
    h->stream = saved;
    return r;
}

// planned batch: the tables of this pass are on the device already
int enqueue_planned_pass(CompressCall& cc, const PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    const flate_hip_plan::Pass& pp = cc.pl->passes[p.index];
    const uint32_t nb = pp.nb;
    cc.prm.n_chunks = p.nc;
    cc.prm.n_blocks = nb;
    cc.prm.stream = 0;
    if (cc.two)  // (sized before the first pass)
        return enqueue_sliced(cc, p.index, p.nc, nb, p.c0, (const fl_chunk*)pp.chunks, (const uint32_t*)pp.blk_chunk, nullptr);
    if ((rc = ensure_block_workspace(h, nb))) return rc;
    return enqueue_pass(h, cc.prm, p.nc, nb, p.c0, (const fl_chunk*)pp.chunks, (const uint32_t*)pp.blk_chunk, nullptr, cc.d_in, cc.d_out,
                        cc.d_outlen, cc.d_status);
}

// A pass's input (pinned input) and its tables on their way to the device, and the compute stream of the pass behind them
int upload_pass(CompressCall& cc, PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    hipStream_t st = cc.st;
    const std::vector<uint64_t>& hin = *cc.hin;
    const uint32_t c0 = p.c0, nc = p.nc, nb = p.nb;
    if (cc.pin_in && !p.sliced) {  // this sub-batch's input: in flight while the previous sub-batch is computed
        const uint64_t a = hin[c0], b = hin[c0 + nc];
        if ((rc = xfer_event(h, 4 * p.index, &p.ev_in))) return rc;
        if (b > a)
            HIP_OK(h, hipMemcpyAsync((uint8_t*)h->st_in.p + (a - cc.in_lo), cc.in + a, b - a, hipMemcpyHostToDevice, h->s_in));
        HIP_OK(h, hipEventRecord(p.ev_in, h->s_in));
    }
    cc.prm.n_chunks = nc;
    cc.prm.n_blocks = nb;
    cc.prm.stream = p.stream ? 1u : 0u;
    if (!p.sliced) {
        if ((rc = ensure(h, h->chunks, sizeof(fl_chunk) * nc))) return rc;
        if ((rc = ensure(h, h->blk_chunk, sizeof(uint32_t) * nb))) return rc;
    }
    if (!cc.two && (rc = ensure_block_workspace(h, nb))) return rc;  // (the two-stream path's are sized before the first pass)
    fl_chunk* tab_chunks = (fl_chunk*)h->chunks.p + (p.sliced ? c0 : 0u);
    uint32_t* tab_blk = (uint32_t*)h->blk_chunk.p + (p.sliced ? cc.blk_base : 0u);
    if (p.sliced) {
        if (cc.blk_base + nb > cc.blk_total) return FLATE_HIP_E_LAUNCH;
        cc.blk_base += nb;
        // (through the pinned table buffer: a copy from a pageable vector is staged by the runtime, and the staged copy of
        // sub-batch k + 1 did not start before the way home of sub-batch k was over -- rocprofv3 timeline, round 5)
        fl_chunk* pt_chunks = (fl_chunk*)h->pin_tab.p + c0;
        uint32_t* pt_blk = (uint32_t*)((fl_chunk*)h->pin_tab.p + cc.n_chunks) + (cc.blk_base - nb);
        memcpy(pt_chunks, &cc.chunks[c0], sizeof(fl_chunk) * nc);
        memcpy(pt_blk, p.blk_chunk->data(), sizeof(uint32_t) * nb);
        HIP_OK(h, hipMemcpyAsync(tab_chunks, pt_chunks, sizeof(fl_chunk) * nc, hipMemcpyHostToDevice, h->s_in));
        HIP_OK(h, hipMemcpyAsync(tab_blk, pt_blk, sizeof(uint32_t) * nb, hipMemcpyHostToDevice, h->s_in));
        const uint64_t a = hin[c0], b = hin[c0 + nc];
        if (cc.pin_in && b > a)
            HIP_OK(h, hipMemcpyAsync((uint8_t*)h->st_in.p + (a - cc.in_lo), cc.in + a, b - a, hipMemcpyHostToDevice, h->s_in));
        if ((rc = xfer_event(h, 4 * p.index, &p.ev_in))) return rc;
        HIP_OK(h, hipEventRecord(p.ev_in, h->s_in));
    } else {
        HIP_OK(h, hipMemcpyAsync(tab_chunks, &cc.chunks[c0], sizeof(fl_chunk) * nc, hipMemcpyHostToDevice, st));
        HIP_OK(h, hipMemcpyAsync(tab_blk, p.blk_chunk->data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
    }
    if (!p.sblocks->empty()) {
        if ((rc = ensure(h, h->sblocks, sizeof(fl_sblock) * p.sblocks->size()))) return rc;
        HIP_OK(h, hipMemcpyAsync(h->sblocks.p, p.sblocks->data(), sizeof(fl_sblock) * p.sblocks->size(), hipMemcpyHostToDevice, st));
        p.dsb = (const fl_sblock*)h->sblocks.p;
    }
    // the host vectors must outlive the async copies
    if (!(cc.pin_in || cc.pin_out) || p.stream || cc.planning) HIP_OK(h, hipStreamSynchronize(st));
    const bool alt = cc.two && p.index < cc.slices.sched.size() && cc.slices.sched[p.index].stream != 0;  // every other sub-batch on the second compute stream
    p.stp = alt ? h->s_c2 : st;
    if (p.ev_in) HIP_OK(h, hipStreamWaitEvent(p.stp, p.ev_in, 0));
    p.dch = tab_chunks;
    p.dbc = tab_blk;
    return FLATE_HIP_OK;
}

// keep this pass's tables in the plan; size the workspace now so that planned calls never allocate
int keep_pass_in_plan(CompressCall& cc, const PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    const uint32_t nc = p.nc, nb = p.nb;
    flate_hip_plan::Pass pp;
    pp.nc = nc;
    pp.nb = nb;
    if (hipMalloc(&pp.chunks, sizeof(fl_chunk) * nc) != hipSuccess ||
        hipMalloc(&pp.blk_chunk, sizeof(uint32_t) * std::max(nb, 1u)) != hipSuccess) {
        if (pp.chunks) (void)hipFree(pp.chunks);
        if (pp.blk_chunk) (void)hipFree(pp.blk_chunk);
        return FLATE_HIP_E_ALLOC;
    }
    cc.pl->passes.push_back(pp);  // the plan owns the tables from here on (flate_hip_plan_destroy frees them)
    // (on the call's stream, ahead of the next pass's tables, which overwrite the source there: a device-to-device hipMemcpy
    // runs on the null stream and does not wait for the host, so the next upload could overtake it)
    HIP_OK(h, hipMemcpyAsync(pp.chunks, h->chunks.p, sizeof(fl_chunk) * nc, hipMemcpyDeviceToDevice, cc.st));
    HIP_OK(h, hipMemcpyAsync(pp.blk_chunk, h->blk_chunk.p, sizeof(uint32_t) * nb, hipMemcpyDeviceToDevice, cc.st));
    if (cc.mode >= 4 && (rc = ensure_lz_workspace(h, nc, cc.prm.chain))) return rc;
    return FLATE_HIP_OK;
}

// A pass of streams with preset dictionaries (dict_compress_plan.h decides, this carries out): every stream's history
// and record side by side in the staging workspace (k_dict_stage), the pass's chunks turned into those staged streams,
// its whole-stream tables, and the chunk table of the records alone for the checksum.  The table uploads are waited for
// in upload_pass.
int stage_dict_pass(CompressCall& cc, PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    fl_chunk* ch = &cc.chunks[p.c0];
    const uint32_t nc = p.nc;
    const uint64_t stage_bytes = fl_dictc_stage(ch, &cc.dc->streams[p.c0], nc, p.jobs);
    fl_dictc_staged_chunks(ch, p.jobs.data(), nc, cc.container);
    p.nb = fl_dictc_pass_tables(ch, p.jobs.data(), nc, p.tabs, *p.blk_chunk);
    p.rec_chunks.assign(ch, ch + nc);
    for (uint32_t i = 0; i < nc; i++) {
        p.rec_chunks[i].in_off = p.jobs[i].src;
        p.rec_chunks[i].in_len = p.jobs[i].n;
    }
    if ((rc = ensure(h, h->dcc_stage, stage_bytes)) || (rc = ensure(h, h->dcc_jobs, sizeof(fl_dictc_job) * nc)) ||
        (rc = ensure(h, h->dcc_chunks, sizeof(fl_chunk) * nc)))
        return rc;
    HIP_OK(h, hipMemcpyAsync(h->dcc_jobs.p, p.jobs.data(), sizeof(fl_dictc_job) * nc, hipMemcpyHostToDevice, cc.st));
    HIP_OK(h, hipMemcpyAsync(h->dcc_chunks.p, p.rec_chunks.data(), sizeof(fl_chunk) * nc, hipMemcpyHostToDevice, cc.st));
    {
        ProfScope ps(h, K_DICT_STAGE);
        hipLaunchKernelGGL(k_dict_stage, dim3(nc), dim3(FL_DSTG_THREADS), 0, cc.st, cc.d_in, cc.dc->d_dict,
                           (const fl_dictc_job*)h->dcc_jobs.p, (uint8_t*)h->dcc_stage.p);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// a whole-stream pass: its checksum, its tokenizer (compress_stream_pass), the shared back end
int enqueue_stream_pass(CompressCall& cc, const PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    hipStream_t st = cc.st;
    const uint32_t c0 = p.c0, nc = p.nc, nb = p.nb;
    // (staged streams: the tokenizer and the back end read the staging workspace, the checksum the records where they lie)
    const uint8_t* d_in = p.staged ? (const uint8_t*)h->dcc_stage.p : cc.d_in;
    if (cc.container != 0) {
        ProfScope ps(h, K_CHECKSUM);
        hipLaunchKernelGGL(k_checksum, dim3(nb), dim3(64), 0, st, cc.d_in, p.staged ? (const fl_chunk*)h->dcc_chunks.p : p.dch, p.dbc,
                           p.dsb, cc.prm, h->crc, (uint32_t*)h->cks.p);
    }
    if ((rc = compress_stream_pass(h, d_in, cc.prm, nc, nb, p.tabs, &cc.chunks[c0]))) return rc;
    h->dbg_pass_chunks = nc;
    h->dbg_first_chunk = c0;
    h->dbg_pos_off.clear();
    h->dbg_chunks.assign(cc.chunks.begin() + c0, cc.chunks.begin() + c0 + nc);
    h->dbg_pieces = p.tabs.pieces;
    if ((rc = enqueue_back_end(h, cc.prm, nc, nb, c0, p.dch, p.dbc, p.dsb, d_in, cc.d_out, cc.d_outlen, cc.d_status))) return rc;
    if (p.staged && cc.container == FLATE_HIP_ZLIB) {  // 78 bb and the DICTID in front of what the back end wrote
        hipLaunchKernelGGL(k_dict_header, dim3((nc + 63) / 64), dim3(64), 0, st, p.dch, (const fl_dictc_job*)h->dcc_jobs.p, nc, cc.dc->d_tab,
                           cc.d_out, cc.d_outlen + c0, cc.d_status + c0);
        HIP_OK(h, hipGetLastError());
    }
    if (cc.pinned_passes) {
        // A whole-stream pass keeps its tables at the START of the table buffers (its block count is not known when
        // the slices are laid out), where the slices of the chunk passes lie: its kernels are only enqueued here, so
        // the input stream -- which fills the next chunk pass's slice -- waits for them first.
        hipEvent_t ev_tab;
        if ((rc = xfer_event(h, 4 * p.index + 3, &ev_tab))) return rc;
        HIP_OK(h, hipEventRecord(ev_tab, st));
        HIP_OK(h, hipStreamWaitEvent(h->s_in, ev_tab, 0));
    }
    return FLATE_HIP_OK;
}

// Pinned output: this sub-batch's output slots go home while the next sub-batch is computed
int send_pass_home(CompressCall& cc, const PassRun& p) {
    flate_hip_ctx* h = cc.h;
    int rc;
    const std::vector<uint64_t>& hout = *cc.hout;
    const uint32_t c0 = p.c0, nc = p.nc;
    hipEvent_t ev_out;
    if ((rc = xfer_event(h, 4 * p.index + 1, &ev_out))) return rc;
    HIP_OK(h, hipEventRecord(ev_out, p.stp));
    HIP_OK(h, hipStreamWaitEvent(h->s_out, ev_out, 0));
    const uint64_t a = hout[c0], b = hout[c0 + nc];
    bool len_by_kernel = false;
    if (b > a && cc.zc_out) {
        const fl_rect r = fl_rect_rows(&hout[c0], nc, h->knobs.rect);  // (pass_plan.h: which slots, and why off by default)
        if (r.urows)
            HIP_OK(h, hipMemcpy2DAsync(cc.out + a, r.pitch, cc.d_out + (a - cc.out_shift), r.pitch, r.half, r.urows, hipMemcpyDeviceToHost, h->s_out));
        uint64_t* len_dev = nullptr;  // device view of pin_len + c0 (the mirror path reads the lengths as the passes land)
        if (cc.landing) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, (uint64_t*)h->pin_len.p + c0, 0) == hipSuccess && dp) len_dev = (uint64_t*)dp;
            else (void)hipGetLastError();
        }
        len_by_kernel = len_dev != nullptr;
        hipLaunchKernelGGL(k_copy_slots, dim3(std::min(64u, nc)), dim3(256), 0, h->s_out, cc.d_out,
                           (const uint64_t*)h->st_slot.p + c0, (const uint64_t*)cc.d_outlen + c0, cc.zc_out,
                           (const uint64_t*)h->st_slot.p + c0, nc, r.urows, r.half, len_dev);
        HIP_OK(h, hipGetLastError());
    } else if (b > a) {
        HIP_OK(h, hipMemcpyAsync(cc.out + a, cc.d_out + (a - cc.out_shift), b - a, hipMemcpyDeviceToHost, h->s_out));
    }
    if (cc.landing) {  // this pass's lengths and an event behind its way home
        hipEvent_t ev_done;
        if ((rc = xfer_event(h, 4 * p.index + 2, &ev_done))) return rc;
        if (!len_by_kernel)
            HIP_OK(h, hipMemcpyAsync((uint64_t*)h->pin_len.p + c0, cc.d_outlen + c0, sizeof(uint64_t) * nc, hipMemcpyDeviceToHost, h->s_out));
        HIP_OK(h, hipEventRecord(ev_done, h->s_out));
    }
    return FLATE_HIP_OK;
}

// Every pass is enqueued: the caller's stream behind the second one, the slices of a plan that was just built, the
// mirror emptied as the passes land, a host caller's lengths, statuses and bytes
int finish_call(CompressCall& cc, PassGuard& pass_guard) {
    flate_hip_ctx* h = cc.h;
    int rc;
    hipStream_t st = cc.st;
    const uint32_t n_chunks = cc.n_chunks;
    if (cc.two) {  // the caller's stream behind the second one
        HIP_OK(h, hipEventRecord(h->c2_ev1, h->s_c2));
        HIP_OK(h, hipStreamWaitEvent(st, h->c2_ev1, 0));
        // the caller's stream is behind the second one: from here on nothing of s_c2 outlives the call unseen, and a planned
        // call only enqueues (flate_hip_compress_planned) -- the host waits below only where it did without two streams
        pass_guard.on = cc.pinned_passes;
    }
    // every pass is enqueued and the caller's stream is behind both: the buffers may grow again (copy_out_host below packs
    // a pageable caller's output in a buffer of its own)
    h->ws_fixed = false;
    if (cc.planning && cc.mode >= 4 && !h->knobs.one_stream) {
        // the planned calls will take two streams: their slices now too (if they cannot be had, the calls take one stream)
        fl_two_slices s;
        if (fl_two_from_plan(cc.pl->passes, s) && size_two_slices(h, cc.prm, s.nc, s.nb)) (void)hipGetLastError();
    }
    if (cc.landing) {
        // everything is enqueued: take the passes' output out of the mirror as they land
        for (size_t k = 0; k < cc.pass_c0.size(); k++) {
            const uint32_t a = cc.pass_c0[k], b = k + 1 < cc.pass_c0.size() ? cc.pass_c0[k + 1] : n_chunks;
            hipEvent_t ev_done;
            if ((rc = xfer_event(h, 4 * k + 2, &ev_done))) return rc;
            HIP_OK(h, hipEventSynchronize(ev_done));
            memcpy(cc.out_len + a, (const uint64_t*)h->pin_len.p + a, sizeof(uint64_t) * (b - a));
            cc.mirror->copy_out(a, b - a);
        }
    }
    if (cc.memkind == FLATE_HIP_MEM_HOST) {
        HIP_OK(h, hipMemcpyAsync(cc.out_len, cc.d_outlen, sizeof(uint64_t) * n_chunks, hipMemcpyDeviceToHost, st));
        HIP_OK(h, hipMemcpyAsync(cc.status, cc.d_status, sizeof(int32_t) * n_chunks, hipMemcpyDeviceToHost, st));
        HIP_OK(h, hipStreamSynchronize(st));
        if (cc.pin_out)
            HIP_OK(h, hipStreamSynchronize(h->s_out));
        else if ((rc = copy_out_host(h, cc.d_out, cc.d_outlen, n_chunks, *cc.hout, cc.out_shift, cc.out, cc.out_len)))
            return rc;
    } else if (h->sync && !h->join) {  // (the pieces of a joined call: the call goes on behind them)
        HIP_OK(h, hipStreamSynchronize(st));
    }
    return FLATE_HIP_OK;
}

int compress_impl(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks, int container,
                  int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, int memkind,
                  const FlushSpec* fs, flate_hip_plan* pl, Mirror* mirror, const DictCall* dc, const JoinCall* jc) {
    const bool planning = pl && !pl->ready;
    if (!h || (!pl && !dc && !jc && (!in_off || !out_off)) || (!planning && (!out_len || !status))) return FLATE_HIP_E_INVALID_ARG;
    if (container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    // The record is declared before the guards, so whatever way the call ends the guards' destructors run first, in this
    // order, and the record's vectors -- which copies on the input stream may still read -- are freed after them:
    // ws_fixed (ensure() may grow buffers again), then pass_guard (the streams are waited for, ck_pending is reset),
    // then ms_guard (the caller's stream waits for the slot clearing).
    CompressCall cc;
    if (!level_args(mode, cc.prm)) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (n_chunks == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    cc.prm.container = container;
    cc.prm.mode = mode;
    cc.prm.flags = (h->flags & FLATE_HIP_DEFLATE_REPAIR_Q1) ? FL_PRM_REPAIR_Q1 : 0u;
    cc.h = h;
    cc.in = in;
    cc.out = out;
    cc.out_len = out_len;
    cc.status = status;
    cc.n_chunks = n_chunks;
    cc.container = container;
    cc.mode = mode;
    cc.memkind = memkind;
    cc.fs = fs;
    cc.dc = dc;
    cc.pl = pl;
    cc.planning = planning;
    cc.planned_run = pl && pl->ready;
    cc.mirror = mirror;
    cc.st = h->stream;

    int rc = 0;
    if (!pl && !dc && !jc) {
        rc = fetch_offsets(h, in_off, n_chunks, memkind, cc.hin_);
        if (rc) return rc;
        rc = fetch_offsets(h, out_off, n_chunks, memkind, cc.hout_);
        if (rc) return rc;
    }
    cc.hin = pl ? &pl->hin : dc ? &dc->hin : jc ? &jc->hin : &cc.hin_;
    cc.hout = pl ? &pl->hout : dc ? &dc->hout : jc ? &jc->hout : &cc.hout_;
    cc.in_lo = (*cc.hin)[0], cc.in_hi = (*cc.hin)[n_chunks];
    cc.out_lo = (*cc.hout)[0], cc.out_hi = (*cc.hout)[n_chunks];

    bool mirrored = false;
    rc = run_on_mirrors(cc, in_off, out_off, &mirrored);
    if (rc || mirrored) return rc;
    if ((rc = stage_host_buffers(cc))) return rc;
    // chunk table + initial status
    if (!fl_chunk_table(cc.hin->data(), cc.hout->data(), n_chunks, cc.in_shift, cc.out_shift, mode, fs, cc.chunks)) return FLATE_HIP_E_INVALID_ARG;
    if (!planning) {
        HIP_OK(h, hipMemsetAsync(cc.d_outlen, 0, sizeof(uint64_t) * n_chunks, cc.st));
        HIP_OK(h, hipMemsetAsync(cc.d_status, 0, sizeof(int32_t) * n_chunks, cc.st));
    }
    MsGuard ms_guard{h};
    if ((rc = clear_slots(cc))) return rc;

    // (pass_plan.h: the kinds of pass, the sub-batch size, the merged tail, the ramp)
    cc.pcfg.n_chunks = n_chunks;
    cc.pcfg.host_pass_chunks = h->knobs.host_pass_chunks;
    cc.pcfg.max_pass_chunks = h->knobs.max_pass_chunks;
    cc.pcfg.pinned = cc.pin_in || cc.pin_out;  // (never with a plan: planned batches are device memory)
    cc.pcfg.ramp = !h->knobs.no_ramp;
    cc.pcfg.planned = pl != nullptr;
    if ((rc = prepare_pinned_tables(cc))) return rc;
    PassGuard pass_guard{h, cc.pinned_passes};
    setup_two_streams(cc);
    pass_guard.on = cc.pinned_passes || cc.two;
    WsFixed ws_fixed{h};
    h->ws_fixed = cc.two;
    if (cc.two) {
        // the second stream behind what the caller's stream holds so far (the cleared lengths and statuses)
        HIP_OK(h, hipEventRecord(h->c2_ev0, cc.st));
        HIP_OK(h, hipStreamWaitEvent(h->s_c2, h->c2_ev0, 0));
        if (h->ms_pending) HIP_OK(h, hipStreamWaitEvent(h->s_c2, h->ms_ev1, 0));  // ... and behind the clearing of the slots
    }
    cc.landing = cc.pin_out && mirror;
    if (cc.landing && !pin_grow(h->pin_len, sizeof(uint64_t) * (size_t)n_chunks, sizeof(uint64_t) * ((size_t)n_chunks + n_chunks / 4 + 64)))
        return FLATE_HIP_E_ALLOC;

    size_t pass_count = 0;
    for (uint32_t c0 = 0, nc = 0; c0 < n_chunks; c0 += nc) {
        fl_pass_pick pk;
        bool staged = false;
        if (dc) {  // (dict_compress_plan.h: the streams with a dictionary in passes of their own)
            const fl_dictc_pick dpk = fl_dictc_pass_next(cc.pcfg, cc.chunks.data(), dc->streams.data(), c0, pass_count, mode,
                                                         h->knobs.stream_pass_bytes, FL_DICTC_PASS_STREAMS);
            pk.nc = dpk.nc;
            pk.stream = dpk.kind != FL_DICTC_CHUNK;
            staged = dpk.kind == FL_DICTC_STAGED;
        } else {
            pk = fl_pass_next(cc.pcfg, cc.chunks.data(), c0, pass_count, mode, fs != nullptr, h->knobs.stream_pass_bytes);
        }
        nc = pk.nc;
        if (pl && pk.stream) return FLATE_HIP_E_UNSUPPORTED;  // (whole-stream passes build more tables per call)
        PassRun p;
        p.c0 = c0;
        p.nc = nc;
        p.index = pass_count++;
        p.stream = pk.stream;
        p.staged = staged;
        p.sliced = cc.pinned_passes && !pk.stream;
        if (mirror) mirror->copy_in(c0, nc);
        cc.pass_c0.push_back(c0);
        if (cc.planned_run) {
            if ((rc = enqueue_planned_pass(cc, p))) return rc;
            continue;
        }
        // block table of this pass (kept until the end of the call: on the pinned path the passes are enqueued without a
        // host wait in between -- 0.27 ms per pass, tools/e2e_probe.py -- and the copies read these vectors)
        cc.keep_blk.emplace_back();
        cc.keep_sb.emplace_back();
        p.blk_chunk = &cc.keep_blk.back();
        p.sblocks = &cc.keep_sb.back();
        if (p.staged) {
            if ((rc = stage_dict_pass(cc, p))) return rc;
        } else {
            p.nb = fl_pass_tables(&cc.chunks[c0], nc, p.stream, mode, fs, p.tabs, *p.blk_chunk, *p.sblocks);
        }
        if ((rc = upload_pass(cc, p))) return rc;
        if (planning) {
            if ((rc = keep_pass_in_plan(cc, p))) return rc;
            continue;
        }
        if (p.stream)
            rc = enqueue_stream_pass(cc, p);
        else if (cc.two)
            rc = enqueue_sliced(cc, p.index, nc, p.nb, c0, p.dch, p.dbc, p.dsb);
        else
            rc = enqueue_pass(h, cc.prm, nc, p.nb, c0, p.dch, p.dbc, p.dsb, cc.d_in, cc.d_out, cc.d_outlen, cc.d_status);
        if (rc) return rc;
        HIP_OK(h, hipGetLastError());
        if (cc.pin_out && (rc = send_pass_home(cc, p))) return rc;
    }
    return finish_call(cc, pass_guard);
}
}  // namespace

extern "C" {

int flate_hip_compress_batch(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                             int container, int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                             int32_t* status, int memkind) {
    return compress_impl(h, in, in_off, n_chunks, container, mode, out, out_off, out_len, status, memkind, nullptr);
}

int flate_hip_compress_flush(flate_hip_handle h, const uint8_t* in, uint64_t n, const uint64_t* flush_pos,
                             uint32_t n_flush, int finish, int container, int mode, uint8_t* out, uint64_t out_cap,
                             uint64_t* out_len, int32_t* status, int memkind) {
    if (!h || !out_len || !status || (n_flush && !flush_pos)) return FLATE_HIP_E_INVALID_ARG;
    if (!(mode == 0 || mode == 1 || (mode >= 4 && mode <= 9))) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST) return FLATE_HIP_E_UNSUPPORTED;
    if (n > 0xfff00000ull) return FLATE_HIP_E_INVALID_ARG;
    uint64_t prev = 0;
    for (uint32_t k = 0; k < n_flush; k++) {
        if (flush_pos[k] < prev || flush_pos[k] > n) return FLATE_HIP_E_INVALID_ARG;
        prev = flush_pos[k];
    }
    // without finish() the stream ends with the marker of the last flush: nothing may follow it
    if (!finish && (n_flush == 0 || flush_pos[n_flush - 1] != n)) return FLATE_HIP_E_INVALID_ARG;
    const uint64_t in_off[2] = {0, n}, out_off[2] = {0, out_cap};
    const FlushSpec fs{flush_pos, n_flush, finish != 0};
    return compress_impl(h, in, in_off, 1, container, mode, out, out_off, out_len, status, memkind, &fs);
}

// Records against preset dictionaries (include/flate_hip.h: what the bytes are; dict_compress_plan.h: every decision).
// Here: the offsets and dict_of on the host, the dictionaries and their table on the device, their Adler-32s; the rest is
// compress_impl with the streams' dictionaries beside it.
int flate_hip_compress_batch_dict(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                  int container, int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                  int32_t* status, int memkind, const uint8_t* dict, const uint64_t* dict_off,
                                  uint32_t n_dicts, const uint32_t* dict_of) {
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    // (what can be said without reading anything back: a wrong container or mode is an error of an empty batch too)
    if (!fl_dictc_args_ok(container, mode, nullptr, 0, nullptr, true, 0) || (n_dicts && !dict_off) || (!dict_of && n_dicts != 1))
        return FLATE_HIP_E_INVALID_ARG;
    if (n_chunks == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    DictCall dc;
    std::vector<uint64_t> hdoff(1, 0);
    std::vector<uint32_t> hof;
    int rc;
    if ((rc = fetch_offsets(h, in_off, n_chunks, memkind, dc.hin))) return rc;
    if ((rc = fetch_offsets(h, out_off, n_chunks, memkind, dc.hout))) return rc;
    if (n_dicts && (rc = fetch_offsets(h, dict_off, n_dicts, memkind, hdoff))) return rc;
    if (dict_of) {
        hof.resize(n_chunks);
        if (memkind == FLATE_HIP_MEM_HOST) {
            memcpy(hof.data(), dict_of, sizeof(uint32_t) * n_chunks);
        } else {
            HIP_OK(h, hipMemcpyAsync(hof.data(), dict_of, sizeof(uint32_t) * n_chunks, hipMemcpyDeviceToHost, st));
            HIP_OK(h, hipStreamSynchronize(st));
        }
    }
    if (!fl_dictc_args_ok(container, mode, hdoff.data(), n_dicts, dict_of ? hof.data() : nullptr, dict_of != nullptr, n_chunks))
        return FLATE_HIP_E_INVALID_ARG;
    const uint64_t d_lo = hdoff[0], d_hi = hdoff[n_dicts];
    if (d_hi > d_lo && !dict) return FLATE_HIP_E_INVALID_ARG;
    std::vector<fl_dict_ent> tab;
    fl_dict_table(hdoff.data(), n_dicts, tab);
    if (memkind == FLATE_HIP_MEM_HOST)  // (the dictionaries are staged from their first byte on)
        for (fl_dict_ent& e : tab) {
            e.start -= d_lo;
            e.end -= d_lo;
        }
    if ((rc = fl_dictc_streams(dc.hin.data(), n_chunks, tab, dict_of ? hof.data() : nullptr, dc.streams))) return rc;
    dc.d_dict = dict;
    if ((rc = ensure(h, h->dc_tab, sizeof(fl_dict_ent) * ((size_t)n_dicts + 1)))) return rc;
    if (memkind == FLATE_HIP_MEM_HOST) {
        if ((rc = ensure(h, h->dc_bytes, (d_hi - d_lo) + 16))) return rc;
        if (d_hi > d_lo) HIP_OK(h, hipMemcpyAsync(h->dc_bytes.p, dict + d_lo, d_hi - d_lo, hipMemcpyHostToDevice, st));
        dc.d_dict = (const uint8_t*)h->dc_bytes.p;
    }
    fl_dict_ent* d_tab = (fl_dict_ent*)h->dc_tab.p;
    dc.d_tab = d_tab;
    if (n_dicts) {
        HIP_OK(h, hipMemcpyAsync(d_tab, tab.data(), sizeof(fl_dict_ent) * n_dicts, hipMemcpyHostToDevice, st));
        HIP_OK(h, hipStreamSynchronize(st));  // (the table is on the host's stack)
        // (the DICTIDs of zlib streams: once per call and dictionary)
        if (container == FLATE_HIP_ZLIB) hipLaunchKernelGGL(k_dict_adler, dim3(n_dicts), dim3(64), 0, st, dc.d_dict, d_tab, n_dicts);
        HIP_OK(h, hipGetLastError());
    }
    return compress_impl(h, in, in_off, n_chunks, container, mode, out, out_off, out_len, status, memkind, nullptr, nullptr, nullptr, &dc);
}

// One gzip / zlib / raw stream from independent pieces (include/flate_hip.h: what the bytes are; join_plan.h: every
// decision).  Here: the offsets on the host, the streams' and pieces' tables on the device, the pieces through
// compress_impl as raw chunks into scratch slots (k_join_open behind every pass: enqueue_pass), then the scan and the pack.
// Host buffers are staged whole.  ji (flate_hip_compress_joined_indexed): the pieces that are points are chosen once the
// streams are laid out, and behind the scan their places are collected (k_join_points) and sent home; the caller waits.
}  // extern "C"
namespace {
int joined_impl(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams, uint32_t piece_bytes, int container,
                int mode, uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, int memkind, JoinIndex* ji) {
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (!fl_join_args_ok(piece_bytes, container, mode)) return FLATE_HIP_E_INVALID_ARG;
    if (n_streams == 0) return FLATE_HIP_OK;
    if (h->join) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    const uint32_t piece = fl_join_piece_bytes(piece_bytes);
    const bool host = memkind == FLATE_HIP_MEM_HOST;
    hipStream_t st = h->stream;
    int rc;
    std::vector<uint64_t> hin, hout;
    if ((rc = fetch_offsets(h, in_off, n_streams, memkind, hin))) return rc;
    if ((rc = fetch_offsets(h, out_off, n_streams, memkind, hout))) return rc;
    const uint64_t in_lo = hin[0], in_hi = hin[n_streams], out_lo = hout[0], out_hi = hout[n_streams];
    if ((in_hi > in_lo && !in) || (out_hi > out_lo && !out)) return FLATE_HIP_E_INVALID_ARG;
    // (host buffers are staged from their first byte on)
    std::vector<fl_join_stream> streams;
    const uint64_t total = fl_join_layout(hin.data(), hout.data(), n_streams, piece, host ? in_lo : 0, host ? out_lo : 0, streams);
    if (total > FL_JOIN_MAX_PIECES) return FLATE_HIP_E_UNSUPPORTED;
    const uint32_t np = (uint32_t)total;
    JoinCall jc;
    std::vector<uint32_t> piece_stream;
    const uint64_t scratch_bytes = fl_join_tables(streams, piece, total, piece_stream, jc.hin, jc.hout);
    jc.container = container;

    if ((rc = ensure(h, h->jn_scratch, scratch_bytes + 16)) || (rc = ensure(h, h->jn_streams, sizeof(fl_join_stream) * (size_t)n_streams)) ||
        (rc = ensure(h, h->jn_pstream, sizeof(uint32_t) * (size_t)np)) || (rc = ensure(h, h->jn_slot, sizeof(uint64_t) * ((size_t)np + 1))) ||
        (rc = ensure(h, h->jn_len, sizeof(uint64_t) * (size_t)np)) || (rc = ensure(h, h->jn_status, sizeof(int32_t) * (size_t)np)) ||
        (rc = ensure(h, h->jn_cks, sizeof(uint32_t) * (size_t)np)) || (rc = ensure(h, h->jn_dst, sizeof(uint64_t) * (size_t)np)) ||
        (rc = ensure(h, h->jn_scks, sizeof(uint32_t) * (size_t)n_streams)))
        return rc;
    std::vector<uint64_t> which_piece;  // ji: the point pieces among the call's pieces
    if (ji) {
        ji->streams = streams;
        ji->n_which.assign(n_streams, 0);
        for (uint32_t i = 0; i < n_streams; i++) {
            const size_t before = ji->which.size();
            fl_idxp_point_pieces(streams[i].n, piece, ji->spacing, ji->which);
            ji->n_which[i] = ji->which.size() - before;
            for (size_t q = before; q < ji->which.size(); q++) which_piece.push_back(streams[i].piece0 + ji->which[q]);
        }
        ji->place.assign(which_piece.size(), 0);
        if ((rc = ensure(h, h->jn_which, sizeof(uint64_t) * which_piece.size())) || (rc = ensure(h, h->jn_place, sizeof(uint64_t) * which_piece.size())))
            return rc;
        HIP_OK(h, hipMemcpyAsync(h->jn_which.p, which_piece.data(), sizeof(uint64_t) * which_piece.size(), hipMemcpyHostToDevice, st));
    }
    const uint8_t* d_in = in;
    uint8_t* d_out = out;
    uint64_t* d_outlen = out_len;
    int32_t* d_status = status;
    if (host) {
        if ((rc = ensure(h, h->st_in, (in_hi - in_lo) + 16)) || (rc = ensure(h, h->st_out, (out_hi - out_lo) + 16)) ||
            (rc = ensure(h, h->st_outlen, sizeof(uint64_t) * (size_t)n_streams)) || (rc = ensure(h, h->st_status, sizeof(int32_t) * (size_t)n_streams)))
            return rc;
        if (in_hi > in_lo) HIP_OK(h, hipMemcpyAsync(h->st_in.p, in + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, st));
        d_in = (const uint8_t*)h->st_in.p;
        d_out = (uint8_t*)h->st_out.p;
        d_outlen = (uint64_t*)h->st_outlen.p;
        d_status = (int32_t*)h->st_status.p;
    }
    HIP_OK(h, hipMemcpyAsync(h->jn_streams.p, streams.data(), sizeof(fl_join_stream) * (size_t)n_streams, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->jn_pstream.p, piece_stream.data(), sizeof(uint32_t) * (size_t)np, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->jn_slot.p, jc.hout.data(), sizeof(uint64_t) * ((size_t)np + 1), hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));  // (the tables are this call's vectors)
    jc.d_piece_stream = (const uint32_t*)h->jn_pstream.p;
    jc.d_streams = (const fl_join_stream*)h->jn_streams.p;
    jc.d_piece_cks = (uint32_t*)h->jn_cks.p;

    // the pieces: raw chunks of the chunk path into their scratch slots, k_join_open behind every pass
    struct JoinGuard {
        flate_hip_ctx* h;
        ~JoinGuard() { h->join = nullptr; }
    } join_guard{h};
    h->join = &jc;
    rc = compress_impl(h, d_in, nullptr, np, FLATE_HIP_RAW, mode, (uint8_t*)h->jn_scratch.p, nullptr, (uint64_t*)h->jn_len.p,
                       (int32_t*)h->jn_status.p, FLATE_HIP_MEM_DEVICE, nullptr, nullptr, nullptr, nullptr, &jc);
    h->join = nullptr;
    if (rc) return rc;
    {
        ProfScope ps(h, K_JOIN_SCAN);
        hipLaunchKernelGGL(k_join_scan, dim3(n_streams), dim3(256), 0, st, jc.d_streams, piece, container, h->crc,
                           (const uint64_t*)h->jn_len.p, (const int32_t*)h->jn_status.p, (const uint32_t*)h->jn_cks.p,
                           (uint64_t*)h->jn_dst.p, d_outlen, d_status, (uint32_t*)h->jn_scks.p);
    }
    {
        ProfScope ps(h, K_JOIN_PACK);
        hipLaunchKernelGGL(k_join_pack, gather_grid(np), dim3(256), 0, st, (const uint8_t*)h->jn_scratch.p, (const uint64_t*)h->jn_slot.p,
                           (const uint64_t*)h->jn_len.p, (const uint64_t*)h->jn_dst.p, jc.d_piece_stream, jc.d_streams, container,
                           (const uint64_t*)d_outlen, (const int32_t*)d_status, (const uint32_t*)h->jn_scks.p, d_out);
    }
    if (ji) {
        ProfScope ps(h, K_JOIN_POINTS);
        const uint64_t nq = ji->place.size();
        hipLaunchKernelGGL(k_join_points, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, (const uint64_t*)h->jn_dst.p,
                           (const uint64_t*)h->jn_which.p, nq, (uint64_t*)h->jn_place.p);
        HIP_OK(h, hipMemcpyAsync(ji->place.data(), h->jn_place.p, sizeof(uint64_t) * nq, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(h, hipGetLastError());
    if (host) {
        HIP_OK(h, hipMemcpyAsync(out_len, d_outlen, sizeof(uint64_t) * (size_t)n_streams, hipMemcpyDeviceToHost, st));
        HIP_OK(h, hipMemcpyAsync(status, d_status, sizeof(int32_t) * (size_t)n_streams, hipMemcpyDeviceToHost, st));
        HIP_OK(h, hipStreamSynchronize(st));
        if ((rc = copy_out_host(h, d_out, d_outlen, n_streams, hout, out_lo, out, out_len))) return rc;
    } else if (h->sync || ji) {
        HIP_OK(h, hipStreamSynchronize(st));
    }
    return FLATE_HIP_OK;
}
}  // namespace
extern "C" {

int flate_hip_compress_joined(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                              uint32_t piece_bytes, int container, int mode, uint8_t* out, const uint64_t* out_off,
                              uint64_t* out_len, int32_t* status, int memkind) {
    return joined_impl(h, in, in_off, n_streams, piece_bytes, container, mode, out, out_off, out_len, status, memkind, nullptr);
}

int flate_hip_decompress_batch(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                               int container, int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                               int32_t* status, uint64_t* consumed, int memkind) {
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (n_chunks == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    std::vector<uint64_t> hin, hout;
    int rc = fetch_offsets(h, in_off, n_chunks, memkind, hin);
    if (rc) return rc;
    rc = fetch_offsets(h, out_off, n_chunks, memkind, hout);
    if (rc) return rc;
    return decompress_core(h, in, hin, n_chunks, container, flags, out, hout, out_len, status, consumed, memkind);
}

// Streams with preset dictionaries: every stream by k_inflate_dict, a wave each (no spans, no workgroup-per-stream kernel).
int flate_hip_decompress_batch_dict(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                    int container, int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                    int32_t* status, uint64_t* consumed, int memkind, const uint8_t* dict,
                                    const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of) {
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (container == FLATE_HIP_GZIP || (n_dicts && !dict_off) || (!dict_of && n_dicts != 1)) return FLATE_HIP_E_INVALID_ARG;
    if (n_chunks == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    std::vector<uint64_t> hin, hout, hdoff(1, 0);
    std::vector<uint32_t> hof;
    int rc;
    if ((rc = fetch_offsets(h, in_off, n_chunks, memkind, hin))) return rc;
    if ((rc = fetch_offsets(h, out_off, n_chunks, memkind, hout))) return rc;
    if (n_dicts && (rc = fetch_offsets(h, dict_off, n_dicts, memkind, hdoff))) return rc;
    if (dict_of) {
        hof.resize(n_chunks);
        if (memkind == FLATE_HIP_MEM_HOST) {
            memcpy(hof.data(), dict_of, sizeof(uint32_t) * n_chunks);
        } else {
            HIP_OK(h, hipMemcpyAsync(hof.data(), dict_of, sizeof(uint32_t) * n_chunks, hipMemcpyDeviceToHost, st));
            HIP_OK(h, hipStreamSynchronize(st));
        }
    }
    if (!fl_dict_args_ok(container, hdoff.data(), n_dicts, dict_of ? hof.data() : nullptr, dict_of != nullptr, n_chunks))
        return FLATE_HIP_E_INVALID_ARG;
    const uint64_t d_lo = hdoff[0], d_hi = hdoff[n_dicts];
    if (d_hi > d_lo && !dict) return FLATE_HIP_E_INVALID_ARG;
    std::vector<fl_dict_ent> tab;
    fl_dict_table(hdoff.data(), n_dicts, tab);

    InflateFrame f(h, memkind, n_chunks);
    f.input(in, hin[0], hin[n_chunks]).output(out, hout[0], hout[n_chunks]).results(out_len, status, consumed);
    const uint32_t what = FRAME_OUT | FRAME_CONSUMED;
    const uint8_t* d_dict = dict;
    const uint32_t* d_of = dict_of;
    if (f.host) {
        if ((rc = reserve_frame(f, what)) || (rc = ensure(h, h->dc_bytes, (d_hi - d_lo) + 16)) ||
            (rc = ensure(h, h->dc_of, sizeof(uint32_t) * n_chunks)) || (rc = stage_frame_whole(f, what)))
            return rc;
        if (d_hi > d_lo) HIP_OK(h, hipMemcpyAsync(h->dc_bytes.p, dict + d_lo, d_hi - d_lo, hipMemcpyHostToDevice, st));
        if (dict_of) HIP_OK(h, hipMemcpyAsync(h->dc_of.p, hof.data(), sizeof(uint32_t) * n_chunks, hipMemcpyHostToDevice, st));
        if ((rc = clear_staged_out(f))) return rc;  // (here, before the tables go up)
        d_dict = (const uint8_t*)h->dc_bytes.p;
        d_of = dict_of ? (const uint32_t*)h->dc_of.p : nullptr;
        for (fl_dict_ent& e : tab) {
            e.start -= d_lo;
            e.end -= d_lo;
        }
    }
    std::vector<fl_chunk> chunks;
    if (!fl_inflate_chunks(hin.data(), hout.data(), n_chunks, f.in_shift, f.out_shift, chunks)) return FLATE_HIP_E_INVALID_ARG;
    if ((rc = ensure(h, h->chunks, sizeof(fl_chunk) * n_chunks)) || (rc = ensure(h, h->dc_tab, sizeof(fl_dict_ent) * (n_dicts + 1))))
        return rc;
    HIP_OK(h, hipMemcpyAsync(h->chunks.p, chunks.data(), sizeof(fl_chunk) * n_chunks, hipMemcpyHostToDevice, st));
    if (n_dicts) HIP_OK(h, hipMemcpyAsync(h->dc_tab.p, tab.data(), sizeof(fl_dict_ent) * n_dicts, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));  // (the tables are on the host's stack)
    h->dbg_span_taken = h->dbg_span_done = h->dbg_par_taken = 0;  // (flate_hip_debug_inflate_paths: every stream by the wave-per-stream kernel)
    if (h->dbg_par_handed.p) HIP_OK(h, hipMemsetAsync(h->dbg_par_handed.p, 0, sizeof(uint32_t), st));
    fl_dict_ent* d_tab = (fl_dict_ent*)h->dc_tab.p;
    if (n_dicts) hipLaunchKernelGGL(k_dict_adler, dim3(n_dicts), dim3(64), 0, st, d_dict, d_tab, n_dicts);
    {
        ProfScope ps(h, K_INFLATE_DICT);
        const auto k = fl_inflate_ring_large(h->knobs.inflate_ring, n_chunks) ? k_inflate_dict<FL_INF_RING_LARGE> : k_inflate_dict<FL_INF_RING_SMALL>;
        hipLaunchKernelGGL(k, dim3(n_chunks), dim3(64), 0, st, f.d_in, (const fl_chunk*)h->chunks.p, container, flags, h->crc, f.d_out,
                           f.d_outlen, f.d_status, f.d_consumed, d_dict, (const fl_dict_ent*)d_tab, d_of);
    }
    HIP_OK(h, hipGetLastError());
    if ((rc = results_home(f, out_len, status, consumed)) || (rc = wait_for_results(f))) return rc;
    return f.host ? copy_out_host(h, f.d_out, f.d_outlen, n_chunks, hout, f.out_shift, out, out_len) : FLATE_HIP_OK;
}

}  // extern "C"

namespace {

// ---- flate_hip_decompress_batch behind its offsets (decompress_core): what a call decides is inflate_plan.h's, the stages
// below carry it out over one record per call.
struct InflateCall {
    flate_hip_ctx* h;
    hipStream_t st;
    const uint8_t* in;  // the caller's buffers and offsets
    uint8_t* out;
    const std::vector<uint64_t>& hin;
    const std::vector<uint64_t>& hout;
    uint32_t n;
    int container, flags;
    InflateFrame f;
    std::vector<fl_chunk> chunks;
    bool pin_io = false;  // host memory, pinned: sub-batches with the copies on s_in / s_out (fl_inflate_pin_io)
    uint32_t sub = 0;     // streams per sub-batch (n: one launch)
    fl_inflate_par par;
    bool large = false;   // the LDS ring of k_inflate
};

int stage_inflate_call(InflateCall& ic) {
    flate_hip_ctx* h = ic.h;
    InflateFrame& f = ic.f;
    const uint32_t what = FRAME_OUT | FRAME_CONSUMED;
    int rc;
    if (f.host) {
        if ((rc = reserve_frame(f, what))) return rc;
        const bool in_pinned = is_pinned_host(ic.in + f.in_lo), out_pinned = in_pinned && is_pinned_host(ic.out + f.out_lo);
        ic.pin_io = fl_inflate_pin_io(in_pinned, out_pinned, f.in_hi - f.in_lo, f.out_hi - f.out_lo, ic.n, h->knobs.host_pass_chunks);
        if (ic.pin_io && ((!h->s_in && create_copy_stream(&h->s_in, true) != hipSuccess) ||
                          (!h->s_out && create_copy_stream(&h->s_out, false) != hipSuccess)))
            return FLATE_HIP_E_ALLOC;
        if ((rc = ic.pin_io ? stage_frame(f, what, nullptr, 0) : stage_frame_whole(f, what))) return rc;
    }
    if (!fl_inflate_chunks(ic.hin.data(), ic.hout.data(), ic.n, f.in_shift, f.out_shift, ic.chunks)) return FLATE_HIP_E_INVALID_ARG;
    if ((rc = upload_chunks(h, ic.chunks)) || (rc = clear_staged_out(f))) return rc;
    h->dbg_span_taken = h->dbg_span_done = h->dbg_par_taken = 0;
    return FLATE_HIP_OK;
}

// A few long streams: each by many workgroups at once (spans); what comes out whole is skipped by the kernels behind it.
int inflate_by_spans(InflateCall& ic) {
    flate_hip_ctx* h = ic.h;
    const InflateFrame& f = ic.f;
    if (ic.pin_io) return FLATE_HIP_OK;
    const int done = try_span_inflate(h, ic.st, f.d_in, ic.chunks, ic.container, ic.flags, f.d_out, f.d_outlen, f.d_status, f.d_consumed);
    if (fl_inflate_pool_release(h->sp_pool.cap)) {
        (void)hipStreamSynchronize(ic.st);
        (void)hipFree(h->sp_pool.p);
        h->ws_bytes -= h->sp_pool.cap;
        h->sp_pool.p = nullptr;
        h->sp_pool.cap = 0;
    }
    if (done < 0) {
        h->last_error = std::string("inflate by spans: ") + hipGetErrorString(hipGetLastError());
        return FLATE_HIP_E_LAUNCH;
    }
    return done > 0 ? upload_chunks(h, ic.chunks) : FLATE_HIP_OK;
}

int choose_inflate_paths(InflateCall& ic) {
    flate_hip_ctx* h = ic.h;
    int rc;
    ic.par = fl_inflate_par_plan(ic.chunks.data(), ic.n, h->knobs.inflate_par, ic.flags);
    if (ic.par.use) {
        if ((rc = ensure(h, h->dbg_par_handed, sizeof(uint32_t)))) return rc;
        HIP_OK(h, hipMemsetAsync(h->dbg_par_handed.p, 0, sizeof(uint32_t), ic.st));
        h->dbg_par_taken += ic.par.taken;
    }
    ic.large = fl_inflate_ring_large(h->knobs.inflate_ring, ic.n);
    if (ic.pin_io) HIP_OK(h, hipStreamSynchronize(h->s_out));  // (nothing of an earlier call may still read st_out)
    ic.sub = ic.pin_io ? fl_inflate_sub_batch(ic.n, h->knobs.host_pass_chunks) : ic.n;
    return FLATE_HIP_OK;
}

// Pinned: every sub-batch's input copy is submitted BEFORE any output copy: an output copy waits for its sub-batch's kernels,
// and an input copy submitted behind it can land in the same in-order DMA queue and wait with it -- then nothing
// overlaps (round 5, profiles/r05_host_path.txt: what happened to the compress path's rectangle copy).
int submit_input_copies(InflateCall& ic) {
    flate_hip_ctx* h = ic.h;
    int rc;
    size_t k = 0;
    for (uint32_t c0 = 0; ic.pin_io && c0 < ic.n; c0 += ic.sub, k++) {
        const uint32_t nc = std::min(ic.sub, ic.n - c0);
        hipEvent_t ev_in;
        if ((rc = xfer_event(h, 2 * k, &ev_in))) return rc;
        const uint64_t a = ic.hin[c0], b = ic.hin[c0 + nc];
        if (b > a) HIP_OK(h, hipMemcpyAsync((uint8_t*)h->st_in.p + (a - ic.f.in_lo), ic.in + a, b - a, hipMemcpyHostToDevice, h->s_in));
        HIP_OK(h, hipEventRecord(ev_in, h->s_in));
    }
    return FLATE_HIP_OK;
}

// nc streams from c0 on: k_inflate_par where the call takes it, then k_inflate over what that left
void launch_inflate(InflateCall& ic, uint32_t c0, uint32_t nc) {
    flate_hip_ctx* h = ic.h;
    const InflateFrame& f = ic.f;
    const fl_chunk* dch = (const fl_chunk*)h->chunks.p + c0;
    uint64_t* d_consumed = f.d_consumed ? f.d_consumed + c0 : nullptr;
    const int32_t* redo_only = nullptr;
    if (ic.par.use) {
        ProfScope ps(h, K_INFLATE_PAR);
        hipLaunchKernelGGL(k_inflate_par, dim3(nc), dim3(FP_THREADS), 0, ic.st, f.d_in, dch, ic.container, ic.flags, ic.par.min_bytes,
                           h->crc, f.d_out, f.d_outlen + c0, f.d_status + c0, d_consumed);
        redo_only = f.d_status + c0;
    }
    ProfScope ps(h, K_INFLATE);
    const auto k = ic.large ? k_inflate<FL_INF_RING_LARGE> : k_inflate<FL_INF_RING_SMALL>;
    hipLaunchKernelGGL(k, dim3(nc), dim3(64), 0, ic.st, f.d_in, dch, ic.container, ic.flags, h->crc, f.d_out, f.d_outlen + c0,
                       f.d_status + c0, d_consumed, redo_only, (uint32_t*)h->dbg_par_handed.p);
}

int run_sub_batches(InflateCall& ic) {
    flate_hip_ctx* h = ic.h;
    int rc;
    size_t k = 0;
    for (uint32_t c0 = 0; c0 < ic.n; c0 += ic.sub, k++) {
        const uint32_t nc = std::min(ic.sub, ic.n - c0);
        if (ic.pin_io) {  // this sub-batch's input: it came in while the sub-batches before it were decoded
            hipEvent_t ev_in;
            if ((rc = xfer_event(h, 2 * k, &ev_in))) return rc;
            HIP_OK(h, hipStreamWaitEvent(ic.st, ev_in, 0));
        }
        launch_inflate(ic, c0, nc);
        HIP_OK(h, hipGetLastError());
        if (ic.pin_io) {  // this sub-batch's output slots go home while the next sub-batch is decoded
            hipEvent_t ev_out;
            if ((rc = xfer_event(h, 2 * k + 1, &ev_out))) return rc;
            HIP_OK(h, hipEventRecord(ev_out, ic.st));
            HIP_OK(h, hipStreamWaitEvent(h->s_out, ev_out, 0));
            const uint64_t a = ic.hout[c0], b = ic.hout[c0 + nc];
            if (b > a) HIP_OK(h, hipMemcpyAsync(ic.out + a, ic.f.d_out + (a - ic.f.out_shift), b - a, hipMemcpyDeviceToHost, h->s_out));
        }
    }
    return FLATE_HIP_OK;
}

// hin / hout are the n_chunks + 1 offsets on the host, everything else is as the entry point got it.
// flate_hip_decompress_members runs it over the members it found (device memory).
int decompress_core(flate_hip_ctx* h, const uint8_t* in, const std::vector<uint64_t>& hin, uint32_t n_chunks, int container,
                    int flags, uint8_t* out, const std::vector<uint64_t>& hout, uint64_t* out_len, int32_t* status,
                    uint64_t* consumed, int memkind) {
    InflateFrame f(h, memkind, n_chunks);
    f.input(in, hin[0], hin[n_chunks]).output(out, hout[0], hout[n_chunks]).results(out_len, status, consumed);
    InflateCall ic{h, h->stream, in, out, hin, hout, n_chunks, container, flags, f};
    int rc;
    if ((rc = stage_inflate_call(ic))) return rc;
    if ((rc = inflate_by_spans(ic))) return rc;
    if ((rc = choose_inflate_paths(ic))) return rc;
    if ((rc = submit_input_copies(ic))) return rc;
    if ((rc = run_sub_batches(ic))) return rc;
    if ((rc = results_home(ic.f, out_len, status, consumed)) || (rc = wait_for_results(ic.f))) return rc;
    if (ic.pin_io) HIP_OK(h, hipStreamSynchronize(h->s_out));
    else if (ic.f.host) return copy_out_host(h, ic.f.d_out, ic.f.d_outlen, n_chunks, hout, ic.f.out_shift, out, out_len);
    return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_decompressed_sizes(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks,
                                 int container, int flags, uint64_t* sizes, int32_t* status, uint64_t* consumed,
                                 int memkind) {
    return sizes_impl(h, in, in_off, n_chunks, container, flags, sizes, status, consumed, memkind, nullptr);
}

int flate_hip_debug_size_paths(flate_hip_handle h, uint64_t counts[2]) {
    if (!h || !counts) return FLATE_HIP_E_INVALID_ARG;
    counts[0] = h->dbg_size_chain;
    counts[1] = h->dbg_size_whole;
    return FLATE_HIP_OK;
}

}  // extern "C"

namespace {

// flate_hip_decompressed_sizes; keep: the span records of its long streams stay with the caller
int sizes_impl(flate_hip_ctx* h, const uint8_t* in, const uint64_t* in_off, uint32_t n_chunks, int container, int flags,
               uint64_t* sizes, int32_t* status, uint64_t* consumed, int memkind, SpanRecords* keep) {
    if (!h || !in_off || !sizes || !status) return FLATE_HIP_E_INVALID_ARG;
    if (container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (n_chunks == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;

    std::vector<uint64_t> hin;
    int rc = fetch_offsets(h, in_off, n_chunks, memkind, hin);
    if (rc) return rc;
    InflateFrame f(h, memkind, n_chunks);
    f.input(in, hin[0], hin[n_chunks]).results(sizes, status, consumed);  // (no output buffer)
    if ((rc = reserve_frame(f, FRAME_CONSUMED)) || (rc = stage_frame_whole(f, FRAME_CONSUMED))) return rc;
    std::vector<fl_chunk> chunks;
    if (!fl_inflate_chunks(hin.data(), nullptr, n_chunks, f.in_shift, 0, chunks)) return FLATE_HIP_E_INVALID_ARG;
    if ((rc = upload_chunks(h, chunks))) return rc;
    h->dbg_size_chain = h->dbg_size_whole = 0;
    // A few long streams: each by many waves at once; what comes out whole is skipped below.
    const int done = size_by_spans(h, st, f.d_in, chunks, container, flags, f.d_outlen, f.d_status, f.d_consumed, keep);
    if (done < 0) {
        h->last_error = std::string("size probe by spans: ") + hipGetErrorString(hipGetLastError());
        return FLATE_HIP_E_LAUNCH;
    }
    if (done > 0 && (rc = upload_chunks(h, chunks))) return rc;
    h->dbg_size_chain = (uint64_t)done;
    h->dbg_size_whole = n_chunks - (uint64_t)done;
    if ((uint32_t)done < n_chunks) {
        ProfScope ps(h, K_INFLATE_SIZE);
        hipLaunchKernelGGL(k_inflate_size<false>, dim3(n_chunks), dim3(64), 0, st, f.d_in, (const fl_chunk*)h->chunks.p, container,
                           flags, f.d_outlen, f.d_status, f.d_consumed, (const fl_size_span*)nullptr, (fl_size_rec*)nullptr);
    }
    HIP_OK(h, hipGetLastError());
    if ((rc = results_home(f, sizes, status, consumed))) return rc;
    return wait_for_results(f);
}

// ---- flate_hip_decompress_members: the call's record and its stages (the rules: member_plan.h)
struct MemberCall {
    flate_hip_ctx* h;
    hipStream_t st;
    uint32_t n;
    int container, flags;
    const std::vector<uint64_t>& hin;  // the caller's offsets
    InflateFrame f;
    const uint64_t* d_inoff;  // the input offsets on the device: the caller's, or vin staged
    uint32_t* d_nmem;
    std::vector<uint64_t> vin, vout;  // the offsets the kernels and decompress_core see
    bool scan = false;                // the members are searched for (gzip), not walked
    uint64_t n_cand = 0;
    fl_member_tiles tiles;
    uint64_t cap = 0;  // entries of all tables together, at most
    uint64_t M = 0;    // ... and as they came back
    std::vector<uint64_t> doff, msize;
    std::vector<uint32_t> mstart;
    std::vector<uint64_t> min_, mout;  // the members as a batch of their own
};

// host memory: the whole call runs on staged copies whose offsets start at 0
int stage_member_call(MemberCall& mc, const std::vector<uint64_t>& hout, bool want_nmem) {
    flate_hip_ctx* h = mc.h;
    InflateFrame& f = mc.f;
    const uint32_t n = mc.n, what = FRAME_OUT | FRAME_CONSUMED | FRAME_NULL_CONSUMED;
    int rc;
    mc.vin = mc.hin;
    mc.vout = hout;
    if (f.host) {
        for (uint32_t i = 0; i <= n; i++) {
            mc.vin[i] -= f.in_lo;
            mc.vout[i] -= f.out_lo;
        }
        if ((rc = reserve_frame(f, what)) || (rc = ensure(h, h->st_inoff, sizeof(uint64_t) * ((size_t)n + 1))) ||
            (rc = ensure(h, h->mb_nmem, sizeof(uint32_t) * n)) || (rc = stage_frame_whole(f, what)))
            return rc;
        HIP_OK(h, hipMemcpyAsync(h->st_inoff.p, mc.vin.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, mc.st));
        if ((rc = clear_staged_out(f))) return rc;
        mc.d_inoff = (const uint64_t*)h->st_inoff.p;
        mc.d_nmem = want_nmem ? (uint32_t*)h->mb_nmem.p : nullptr;
    }
    h->dbg_member[0] = h->dbg_member[1] = h->dbg_member[2] = 0;
    if ((rc = ensure(h, h->mb_taboff, sizeof(uint64_t) * ((size_t)n + 1)))) return rc;
    if ((rc = ensure(h, h->mb_tabn, sizeof(uint64_t) * n))) return rc;
    if ((rc = ensure(h, h->mb_non, sizeof(uint64_t) * n))) return rc;
    return ensure(h, h->mb_denseoff, sizeof(uint64_t) * ((size_t)n + 1));
}

// scan: count the candidates; too many, and the call walks
int count_member_candidates(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    const InflateFrame& f = mc.f;
    const uint64_t lo = mc.vin[0], hi = mc.vin[mc.n];
    int rc;
    mc.scan = mc.container == 1 && h->knobs.member_scan;
    if (!mc.scan || hi <= lo) return FLATE_HIP_OK;
    if (!fl_member_scan_tiles((uint64_t)(uintptr_t)f.d_in, lo, hi, mc.tiles)) return FLATE_HIP_E_INVALID_ARG;
    const uint64_t n_tiles = mc.tiles.n_tiles;
    if ((rc = ensure(h, h->mb_tiles, sizeof(uint64_t) * (n_tiles + 1)))) return rc;
    if ((rc = ensure(h, h->mb_tileoff, sizeof(uint64_t) * (n_tiles + 1)))) return rc;
    {
        ProfScope ps(h, K_MEMBER_SCAN);
        hipLaunchKernelGGL(k_member_scan<false>, dim3((uint32_t)n_tiles), dim3(64), 0, mc.st, f.d_in, mc.tiles.rel0, lo, hi, mc.d_inoff,
                           mc.n, (uint64_t*)h->mb_tiles.p, (uint64_t*)nullptr, (fl_chunk*)nullptr, (uint64_t)0);
        hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, mc.st, (const uint64_t*)h->mb_tiles.p, (uint32_t)n_tiles,
                           (uint64_t*)h->mb_tileoff.p);
    }
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, hipMemcpyAsync(&mc.n_cand, (const uint64_t*)h->mb_tileoff.p + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, mc.st));
    HIP_OK(h, hipStreamSynchronize(mc.st));
    if (mc.n_cand > h->knobs.member_candidates) mc.scan = false;
    return FLATE_HIP_OK;
}

// the member tables: the candidates' arrays (scan) or where every stream's table starts (walk), and room for cap entries
int size_member_tables(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    const uint32_t n = mc.n;
    int rc;
    if (mc.scan) {
        mc.cap = fl_member_scan_cap(mc.n_cand, n);
        const size_t nc1 = (size_t)std::max<uint64_t>(mc.n_cand, 1);
        if ((rc = ensure(h, h->mb_cand, sizeof(uint64_t) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_chunks, sizeof(fl_chunk) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_psize, sizeof(uint64_t) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_pstatus, sizeof(int32_t) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_pcons, sizeof(uint64_t) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_succ, sizeof(uint32_t) * nc1))) return rc;
        if ((rc = ensure(h, h->mb_chain, sizeof(uint32_t) * nc1))) return rc;
    } else {
        std::vector<uint64_t> toff((size_t)n + 1);
        mc.cap = fl_member_walk_offsets(mc.hin.data(), n, mc.container, toff.data());
        HIP_OK(h, hipMemcpyAsync(h->mb_taboff.p, toff.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, mc.st));
        HIP_OK(h, hipStreamSynchronize(mc.st));  // (toff leaves scope)
    }
    if ((rc = ensure(h, h->mb_tabstart, sizeof(uint32_t) * mc.cap))) return rc;
    return ensure(h, h->mb_tabsize, sizeof(uint64_t) * mc.cap);
}

// every stream's table: from the chain of its candidates (scan), or member by member (walk)
int scan_or_walk_members(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    const InflateFrame& f = mc.f;
    const uint32_t n = mc.n;
    const uint64_t lo = mc.vin[0], hi = mc.vin[n];
    if (mc.scan) {
        if (mc.n_cand) {
            {
                ProfScope ps(h, K_MEMBER_SCAN);
                hipLaunchKernelGGL(k_member_scan<true>, dim3((uint32_t)mc.tiles.n_tiles), dim3(64), 0, mc.st, f.d_in, mc.tiles.rel0, lo, hi,
                                   mc.d_inoff, n, (uint64_t*)h->mb_tileoff.p, (uint64_t*)h->mb_cand.p, (fl_chunk*)h->mb_chunks.p, mc.n_cand);
            }
            ProfScope ps(h, K_INFLATE_SIZE);
            hipLaunchKernelGGL(k_inflate_size<false>, dim3((uint32_t)mc.n_cand), dim3(64), 0, mc.st, f.d_in, (const fl_chunk*)h->mb_chunks.p,
                               mc.container, mc.flags, (uint64_t*)h->mb_psize.p, (int32_t*)h->mb_pstatus.p, (uint64_t*)h->mb_pcons.p,
                               (const fl_size_span*)nullptr, (fl_size_rec*)nullptr);
        }
        ProfScope ps(h, K_MEMBER_CHAIN);
        hipLaunchKernelGGL(k_member_chain, dim3(n), dim3(64), 0, mc.st, mc.d_inoff, (const uint64_t*)h->mb_cand.p, (uint32_t)mc.n_cand,
                           (const int32_t*)h->mb_pstatus.p, (const uint64_t*)h->mb_pcons.p, (const uint64_t*)h->mb_psize.p,
                           (uint32_t*)h->mb_succ.p, (uint32_t*)h->mb_chain.p, (uint64_t*)h->mb_taboff.p, (uint64_t*)h->mb_tabn.p,
                           (uint32_t*)h->mb_tabstart.p, (uint64_t*)h->mb_tabsize.p, (uint64_t*)h->mb_non.p);
    } else {
        ProfScope ps(h, K_MEMBER_WALK);
        hipLaunchKernelGGL(k_member_walk, dim3(n), dim3(64), 0, mc.st, f.d_in, mc.d_inoff, mc.container, mc.flags,
                           (const uint64_t*)h->mb_taboff.p, (uint64_t*)h->mb_tabn.p, (uint32_t*)h->mb_tabstart.p, (uint64_t*)h->mb_tabsize.p);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// back to back, and home: with the candidates counted the table's size is bounded and it comes with its offsets
int pack_and_fetch_members(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    const uint32_t n = mc.n;
    const uint64_t cap = mc.cap;
    std::vector<uint64_t> non;
    int rc;
    mc.doff.resize((size_t)n + 1);
    if ((rc = ensure(h, h->mb_dstart, sizeof(uint32_t) * cap))) return rc;
    if ((rc = ensure(h, h->mb_dsize, sizeof(uint64_t) * cap))) return rc;
    {
        ProfScope ps(h, K_MEMBER_PACK);
        hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, mc.st, (const uint64_t*)h->mb_tabn.p, n, (uint64_t*)h->mb_denseoff.p);
        hipLaunchKernelGGL(k_member_pack, dim3(n), dim3(64), 0, mc.st, (const uint64_t*)h->mb_taboff.p, (const uint64_t*)h->mb_tabn.p,
                           (const uint32_t*)h->mb_tabstart.p, (const uint64_t*)h->mb_tabsize.p, (const uint64_t*)h->mb_denseoff.p,
                           (uint32_t*)h->mb_dstart.p, (uint64_t*)h->mb_dsize.p);
    }
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, hipMemcpyAsync(mc.doff.data(), h->mb_denseoff.p, sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyDeviceToHost, mc.st));
    if (mc.scan) {
        non.resize(n);
        mc.mstart.resize(cap);
        mc.msize.resize(cap);
        HIP_OK(h, hipMemcpyAsync(non.data(), h->mb_non.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, mc.st));
        HIP_OK(h, hipMemcpyAsync(mc.mstart.data(), h->mb_dstart.p, sizeof(uint32_t) * cap, hipMemcpyDeviceToHost, mc.st));
        HIP_OK(h, hipMemcpyAsync(mc.msize.data(), h->mb_dsize.p, sizeof(uint64_t) * cap, hipMemcpyDeviceToHost, mc.st));
    }
    HIP_OK(h, hipStreamSynchronize(mc.st));
    mc.M = mc.doff[n];
    if (!fl_member_count_ok(mc.M, n, cap)) {
        h->last_error = "member table: " + std::to_string(mc.M) + " members of " + std::to_string(n) + " streams";
        return FLATE_HIP_E_LAUNCH;
    }
    if (!mc.scan) {
        mc.mstart.resize(mc.M);
        mc.msize.resize(mc.M);
        HIP_OK(h, hipMemcpyAsync(mc.mstart.data(), h->mb_dstart.p, sizeof(uint32_t) * mc.M, hipMemcpyDeviceToHost, mc.st));
        HIP_OK(h, hipMemcpyAsync(mc.msize.data(), h->mb_dsize.p, sizeof(uint64_t) * mc.M, hipMemcpyDeviceToHost, mc.st));
        HIP_OK(h, hipStreamSynchronize(mc.st));
        h->dbg_member[1] = n;
        return FLATE_HIP_OK;
    }
    uint64_t on = 0;
    for (uint32_t i = 0; i < n; i++) on += non[i];
    h->dbg_member[0] = n;
    h->dbg_member[2] = mc.n_cand - on;
    return FLATE_HIP_OK;
}

// the members as a batch of their own: a contiguous partition of the input and of the slots
int partition_members(MemberCall& mc) {
    mc.min_.resize((size_t)mc.M + 1);
    mc.mout.resize((size_t)mc.M + 1);
    const fl_member_verdict v = fl_member_partition(mc.doff.data(), mc.mstart.data(), mc.msize.data(), mc.vin.data(), mc.vout.data(),
                                                    mc.n, mc.min_.data(), mc.mout.data());
    if (v.fault == FL_MEM_TAB_OK) return FLATE_HIP_OK;
    mc.h->last_error = "member table: stream " + std::to_string(v.stream) +
                       (v.fault == FL_MEM_TAB_NO_FIRST ? " does not start with a member" : " is out of order");
    return FLATE_HIP_E_LAUNCH;
}

int decode_members(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    int rc;
    if ((rc = ensure(h, h->mb_outlen, sizeof(uint64_t) * mc.M))) return rc;
    if ((rc = ensure(h, h->mb_status, sizeof(int32_t) * mc.M))) return rc;
    if ((rc = ensure(h, h->mb_cons, sizeof(uint64_t) * mc.M))) return rc;
    return decompress_core(h, mc.f.d_in, mc.min_, (uint32_t)mc.M, mc.container, mc.flags, mc.f.d_out, mc.mout, (uint64_t*)h->mb_outlen.p,
                           (int32_t*)h->mb_status.p, (uint64_t*)h->mb_cons.p, FLATE_HIP_MEM_DEVICE);
}

int fold_members(MemberCall& mc) {
    flate_hip_ctx* h = mc.h;
    {
        ProfScope ps(h, K_MEMBER_FOLD);
        hipLaunchKernelGGL(k_member_fold, dim3(mc.n), dim3(64), 0, mc.st, (const uint64_t*)h->mb_denseoff.p,
                           (const uint64_t*)h->mb_outlen.p, (const int32_t*)h->mb_status.p, (const uint64_t*)h->mb_cons.p, mc.f.d_outlen,
                           mc.f.d_status, mc.f.d_consumed, mc.d_nmem);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

// The members of every stream, found on the device (kernels_members.h), decoded by decompress_core as streams of their own
// and folded back.  The host waits for the offsets, for the candidate count (scan) or the member count (walk), and for
// the member table; then decompress_core waits as it does for any batch on device memory.
int flate_hip_decompress_members(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                                 int container, int flags, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                                 int32_t* status, uint64_t* consumed, uint32_t* n_members, int memkind) {
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (n_streams == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    const uint32_t n = n_streams;
    std::vector<uint64_t> hin, hout;
    int rc;
    if ((rc = fetch_offsets(h, in_off, n, memkind, hin)) || (rc = fetch_offsets(h, out_off, n, memkind, hout))) return rc;
    if (fl_inflate_oversize(hin.data(), n) != n) return FLATE_HIP_E_INVALID_ARG;
    InflateFrame f(h, memkind, n);
    f.input(in, hin[0], hin[n]).output(out, hout[0], hout[n]).results(out_len, status, consumed);
    MemberCall mc{h, h->stream, n, container, flags, hin, f, in_off, n_members};
    if ((rc = stage_member_call(mc, hout, n_members != nullptr))) return rc;
    if ((rc = count_member_candidates(mc))) return rc;
    if ((rc = size_member_tables(mc))) return rc;
    if ((rc = scan_or_walk_members(mc))) return rc;
    if ((rc = pack_and_fetch_members(mc))) return rc;
    if ((rc = partition_members(mc))) return rc;
    if ((rc = decode_members(mc))) return rc;
    if ((rc = fold_members(mc))) return rc;
    if ((rc = results_home(mc.f, out_len, status, consumed))) return rc;
    if (mc.f.host && n_members) HIP_OK(h, hipMemcpyAsync(n_members, mc.d_nmem, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, h->stream));
    if ((rc = wait_for_results(mc.f))) return rc;
    return mc.f.host ? copy_out_host(h, mc.f.d_out, mc.f.d_outlen, n, hout, mc.f.out_shift, out, out_len) : FLATE_HIP_OK;
}

int flate_hip_debug_member_paths(flate_hip_handle h, uint64_t counts[3]) {
    if (!h || !counts) return FLATE_HIP_E_INVALID_ARG;
    for (int i = 0; i < 3; i++) counts[i] = h->dbg_member[i];
    return FLATE_HIP_OK;
}

int flate_hip_gather_streams(flate_hip_handle h, const uint8_t* out, const uint64_t* out_off, const uint64_t* out_len,
                             uint32_t n_chunks, uint8_t* dst, uint64_t* dst_off) {
    if (!h || !out || !out_off || !out_len || !dst || !dst_off) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    {
        ProfScope ps(h, K_GATHER);
        hipLaunchKernelGGL(k_scan_lens, dim3(1), dim3(1024), 0, st, out_len, n_chunks, dst_off);
        if (n_chunks)
            hipLaunchKernelGGL(k_gather_copy, gather_grid(n_chunks), dim3(256), 0, st, out, out_off, out_len, dst,
                               (const uint64_t*)dst_off);
    }
    HIP_OK(h, hipGetLastError());
    if (h->sync) HIP_OK(h, hipStreamSynchronize(st));
    return FLATE_HIP_OK;
}

int flate_hip_set_flags(flate_hip_handle h, uint32_t flags) {
    if (!h || (flags & ~(uint32_t)FLATE_HIP_DEFLATE_REPAIR_Q1)) return FLATE_HIP_E_INVALID_ARG;
    h->flags = flags;
    return FLATE_HIP_OK;
}

int flate_hip_debug_phase_cycles(flate_hip_handle h, uint64_t* out, int n) {
    if (!h || !out || n <= 0) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return FLATE_HIP_E_LAUNCH;
    uint64_t tmp[FL_PROF_SLOTS];
    if (hipMemcpyFromSymbol(tmp, HIP_SYMBOL(g_fl_prof), sizeof tmp) != hipSuccess) return FLATE_HIP_E_LAUNCH;
    for (int i = 0; i < n && i < FL_PROF_SLOTS; i++) out[i] = tmp[i];
    return FLATE_HIP_OK;
}

int64_t flate_hip_debug_tokens(flate_hip_handle h, uint32_t chunk, uint32_t* tokens, uint64_t cap) {
    if (!h || !tokens) return FLATE_HIP_E_INVALID_ARG;
    if (chunk < h->dbg_first_chunk || chunk >= h->dbg_first_chunk + h->dbg_pass_chunks) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    const uint32_t local = chunk - h->dbg_first_chunk;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return FLATE_HIP_E_LAUNCH;
    if (!h->dbg_pieces.empty()) {
        // whole-stream pass: the token lists of the chunk's pieces, one after the other
        const fl_chunk& c = h->dbg_chunks[local];
        uint64_t total = 0;
        for (uint32_t i = 0; i < c.n_piece; i++) {
            const fl_piece& pc = h->dbg_pieces[c.piece0 + i];
            uint32_t m = 0;
            if (hipMemcpy(&m, (uint32_t*)h->ntok.p + c.piece0 + i, sizeof m, hipMemcpyDeviceToHost) != hipSuccess)
                return FLATE_HIP_E_LAUNCH;
            if (total + m <= cap && m &&
                hipMemcpy(tokens + total, (uint32_t*)h->tokens.p + c.pos_off + pc.start, (size_t)m * sizeof(uint32_t),
                          hipMemcpyDeviceToHost) != hipSuccess)
                return FLATE_HIP_E_LAUNCH;
            total += m;
        }
        return (int64_t)total;
    }
    uint32_t n = 0;
    if (hipMemcpy(&n, (uint32_t*)h->ntok.p + local, sizeof n, hipMemcpyDeviceToHost) != hipSuccess)
        return FLATE_HIP_E_LAUNCH;
    const uint64_t k = std::min<uint64_t>(n, cap);
    if (k && hipMemcpy(tokens, (uint32_t*)h->tokens.p + h->dbg_pos_off[local], k * sizeof(uint32_t),
                       hipMemcpyDeviceToHost) != hipSuccess)
        return FLATE_HIP_E_LAUNCH;
    return (int64_t)n;
}

int flate_hip_debug_write_block(flate_hip_handle h, const uint32_t* tokens, uint32_t n_tokens, const uint8_t* input,
                                uint32_t input_len, int eof, int dynamic_only, uint8_t* out, uint64_t out_cap,
                                uint64_t* out_len) {
    if (!h || !out || !out_len || (n_tokens && !tokens) || n_tokens > FL_MAX_TOKENS) return FLATE_HIP_E_INVALID_ARG;
    const bool has_input = input != nullptr;
    if (has_input && input_len > 0xfffffff0u) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    int rc;
    const uint32_t in_len = has_input ? input_len : 0u;
    const uint64_t cap4 = (out_cap + 3) & ~3ull;
    if ((rc = ensure(h, h->chunks, sizeof(fl_chunk)))) return rc;
    if ((rc = ensure(h, h->blk_chunk, sizeof(uint32_t)))) return rc;
    if ((rc = ensure(h, h->plans, sizeof(fl_block_plan)))) return rc;
    if ((rc = ensure(h, h->hist, sizeof(uint32_t) * 320))) return rc;
    if ((rc = ensure(h, h->cks, sizeof(uint32_t) * 2))) return rc;
    if ((rc = ensure(h, h->tokens, sizeof(uint32_t) * ((size_t)n_tokens + 1)))) return rc;
    if ((rc = ensure(h, h->st_in, (size_t)in_len + 16))) return rc;
    if ((rc = ensure(h, h->st_out, cap4 + 16))) return rc;
    if ((rc = ensure(h, h->st_outlen, sizeof(uint64_t)))) return rc;
    if ((rc = ensure(h, h->st_status, sizeof(int32_t)))) return rc;
    fl_chunk ck{};
    ck.in_off = 0;
    ck.out_off = 0;
    ck.out_cap = out_cap;
    ck.in_len = in_len;
    ck.n_blocks = 1;
    fl_block_plan plan{};
    plan.valid = 1;
    plan.tok_count = n_tokens;
    plan.in_len = has_input ? in_len : FL_NO_INPUT;  // Zig null: the block cannot be stored
    plan.final_block = eof ? 1u : 0u;
    const uint32_t zero = 0;
    fl_params prm{};
    level_args(6, prm);
    prm.n_chunks = 1;
    prm.n_blocks = 1;
    prm.container = 0;
    prm.mode = 6;
    prm.stream = 1;  // plain block numbering in k_plan
    prm.plan_dynamic_only = dynamic_only ? 1u : 0u;
    HIP_OK(h, hipMemcpyAsync(h->chunks.p, &ck, sizeof ck, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->blk_chunk.p, &zero, sizeof zero, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->plans.p, &plan, sizeof plan, hipMemcpyHostToDevice, st));
    if (n_tokens)
        HIP_OK(h, hipMemcpyAsync(h->tokens.p, tokens, sizeof(uint32_t) * n_tokens, hipMemcpyHostToDevice, st));
    if (in_len) HIP_OK(h, hipMemcpyAsync(h->st_in.p, input, in_len, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemsetAsync(h->st_out.p, 0, cap4 + 16, st));
    HIP_OK(h, hipStreamSynchronize(st));  // the host structs must outlive the async copies
    hipLaunchKernelGGL(k_dbg_token_hist, dim3(1), dim3(256), 0, st, (const uint32_t*)h->tokens.p,
                       (const fl_chunk*)h->chunks.p, (const uint32_t*)h->blk_chunk.p, (const fl_block_plan*)h->plans.p,
                       (uint32_t*)h->hist.p);
    hipLaunchKernelGGL(k_plan, dim3(1), dim3(64 * FL_PLAN_WAVES), 0, st, (const fl_chunk*)h->chunks.p,
                       (const uint32_t*)h->blk_chunk.p, (const fl_sblock*)nullptr, prm, (const uint32_t*)h->hist.p,
                       (fl_block_plan*)h->plans.p);
    hipLaunchKernelGGL(k_offsets, dim3(1), dim3(64), 0, st, (const fl_chunk*)h->chunks.p, prm, h->crc,
                       (fl_block_plan*)h->plans.p, (const uint32_t*)h->cks.p, (uint8_t*)h->st_out.p,
                       (uint64_t*)h->st_outlen.p, (int32_t*)h->st_status.p);
    hipLaunchKernelGGL(k_encode<true>, dim3(1), dim3(64 * FL_ENC_WAVES), 0, st, (const uint8_t*)h->st_in.p,
                       (const fl_chunk*)h->chunks.p, (const uint32_t*)h->blk_chunk.p,
                       (const fl_block_plan*)h->plans.p, (const uint32_t*)h->tokens.p, (uint32_t*)h->st_out.p);
    HIP_OK(h, hipGetLastError());
    int32_t status = 0;
    HIP_OK(h, hipMemcpyAsync(out_len, h->st_outlen.p, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(&status, h->st_status.p, sizeof status, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    if (status != 0) return FLATE_HIP_E_INVALID_ARG;  // out_cap too small
    if (*out_len) HIP_OK(h, hipMemcpy(out, h->st_out.p, *out_len, hipMemcpyDeviceToHost));
    return FLATE_HIP_OK;
}

int flate_hip_debug_write_blocks(flate_hip_handle h, uint32_t n, const uint32_t* tokens, const uint64_t* tok_off,
                                 const uint8_t* input, const uint64_t* in_off, const uint8_t* has_input,
                                 const uint8_t* eof, int dynamic_only, int encoder, int paired, uint8_t* out,
                                 uint64_t out_cap, const uint64_t* slot_off, const uint64_t* slot_cap,
                                 uint64_t* out_len) {
    if (!h || !n || n > 65536u || !tok_off || !in_off || !has_input || !eof || !out || !slot_off || !slot_cap || !out_len)
        return FLATE_HIP_E_INVALID_ARG;
    if ((encoder != 0 && encoder != 1) || (out_cap & 3) || ((uintptr_t)out & 3)) return FLATE_HIP_E_INVALID_ARG;
    if ((tok_off[n] && !tokens) || (in_off[n] && !input)) return FLATE_HIP_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; i++) {
        if (tok_off[i + 1] < tok_off[i] || tok_off[i + 1] - tok_off[i] > FL_MAX_TOKENS) return FLATE_HIP_E_INVALID_ARG;
        if (in_off[i + 1] < in_off[i] || in_off[i + 1] - in_off[i] > 0xfffffff0u) return FLATE_HIP_E_INVALID_ARG;
        if (slot_cap[i] > out_cap || slot_off[i] > out_cap - slot_cap[i]) return FLATE_HIP_E_INVALID_ARG;
    }
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    int rc;
    const uint32_t per = paired ? 2u : 1u, nb = n * per;
    if ((rc = ensure(h, h->chunks, sizeof(fl_chunk) * n))) return rc;
    if ((rc = ensure(h, h->blk_chunk, sizeof(uint32_t) * nb))) return rc;
    if ((rc = ensure(h, h->plans, sizeof(fl_block_plan) * nb))) return rc;
    if ((rc = ensure(h, h->hist, sizeof(uint32_t) * 320 * nb))) return rc;
    if ((rc = ensure(h, h->cks, sizeof(uint32_t) * 2 * nb))) return rc;
    if ((rc = ensure(h, h->tokens, sizeof(uint32_t) * ((size_t)tok_off[n] + 1)))) return rc;
    if ((rc = ensure(h, h->st_in, (size_t)in_off[n] + 16))) return rc;
    if ((rc = ensure(h, h->st_out, out_cap + 16))) return rc;
    if ((rc = ensure(h, h->st_outlen, sizeof(uint64_t) * n))) return rc;
    if ((rc = ensure(h, h->st_status, sizeof(int32_t) * n))) return rc;
    std::vector<fl_chunk> cks(n);
    std::vector<uint32_t> bc(nb);
    std::vector<fl_block_plan> plans(nb);  // (value-initialised: valid = 0 in every second slot of the paired layout)
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t in_len = (uint32_t)(in_off[i + 1] - in_off[i]);
        fl_chunk& ck = cks[i];
        ck = fl_chunk{};
        ck.in_off = in_off[i];
        ck.out_off = slot_off[i];
        ck.out_cap = slot_cap[i];
        ck.pos_off = tok_off[i];
        ck.in_len = in_len;
        ck.first_block = i * per;
        ck.n_blocks = per;
        for (uint32_t k = 0; k < per; k++) bc[i * per + k] = i;
        fl_block_plan& plan = plans[i * per];
        plan.valid = 1;
        plan.tok_count = (uint32_t)(tok_off[i + 1] - tok_off[i]);
        plan.in_len = has_input[i] ? in_len : FL_NO_INPUT;  // Zig null: the block cannot be stored
        plan.final_block = eof[i] ? 1u : 0u;
    }
    fl_params prm{};
    level_args(6, prm);
    prm.n_chunks = n;
    prm.n_blocks = nb;
    prm.container = 0;
    prm.mode = 6;
    prm.stream = paired ? 0u : 1u;  // paired: k_plan visits the slots in the chunk path's order; else plain numbering
    prm.plan_dynamic_only = dynamic_only ? 1u : 0u;
    HIP_OK(h, hipMemcpyAsync(h->chunks.p, cks.data(), sizeof(fl_chunk) * n, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->blk_chunk.p, bc.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->plans.p, plans.data(), sizeof(fl_block_plan) * nb, hipMemcpyHostToDevice, st));
    if (tok_off[n])
        HIP_OK(h, hipMemcpyAsync(h->tokens.p, tokens, sizeof(uint32_t) * tok_off[n], hipMemcpyHostToDevice, st));
    if (in_off[n]) HIP_OK(h, hipMemcpyAsync(h->st_in.p, input, in_off[n], hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemsetAsync(h->st_out.p, 0, out_cap + 16, st));
    HIP_OK(h, hipStreamSynchronize(st));  // the host tables must outlive the async copies
    const fl_chunk* dch = (const fl_chunk*)h->chunks.p;
    const uint32_t* dbc = (const uint32_t*)h->blk_chunk.p;
    fl_block_plan* dpl = (fl_block_plan*)h->plans.p;
    hipLaunchKernelGGL(k_dbg_token_hist, dim3(nb), dim3(256), 0, st, (const uint32_t*)h->tokens.p, dch, dbc,
                       (const fl_block_plan*)dpl, (uint32_t*)h->hist.p);
    hipLaunchKernelGGL(k_plan, dim3((nb + FL_PLAN_WAVES - 1) / FL_PLAN_WAVES), dim3(64 * FL_PLAN_WAVES), 0, st, dch, dbc,
                       (const fl_sblock*)nullptr, prm, (const uint32_t*)h->hist.p, dpl);
    hipLaunchKernelGGL(k_offsets, dim3(n), dim3(64), 0, st, dch, prm, h->crc, dpl, (const uint32_t*)h->cks.p,
                       (uint8_t*)h->st_out.p, (uint64_t*)h->st_outlen.p, (int32_t*)h->st_status.p);
    if (encoder == 1)
        hipLaunchKernelGGL(k_encode_wave, dim3((nb + FL_ENC_WAVES - 1) / FL_ENC_WAVES), dim3(64 * FL_ENC_WAVES), 0, st,
                           (const uint8_t*)h->st_in.p, dch, dbc, (const fl_block_plan*)dpl, (const uint32_t*)h->tokens.p,
                           (uint32_t*)h->st_out.p, nb, paired ? 1u : 0u);
    else
        hipLaunchKernelGGL(k_encode<true>, dim3(nb), dim3(64 * FL_ENC_WAVES), 0, st, (const uint8_t*)h->st_in.p, dch, dbc,
                           (const fl_block_plan*)dpl, (const uint32_t*)h->tokens.p, (uint32_t*)h->st_out.p);
    HIP_OK(h, hipGetLastError());
    std::vector<int32_t> status(n);
    HIP_OK(h, hipMemcpyAsync(out_len, h->st_outlen.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(status.data(), h->st_status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(out, h->st_out.p, out_cap, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++)
        if (status[i] != 0) return FLATE_HIP_E_INVALID_ARG;  // a slot too small
    return FLATE_HIP_OK;
}

// ---- multi-GPU: the local shard through the single-GPU path, then the reassembly over RCCL ----
// RCCL is not linked: the entry points bind to the RCCL the process already uses (the communicator
// the caller hands over was made by it), or load librccl.so when none is loaded yet.
namespace {
struct RcclApi {
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool ok = false;
};
const RcclApi& rccl() {
    static RcclApi api = [] {
        RcclApi a;
        void* lib = RTLD_DEFAULT;
        if (!dlsym(lib, "ncclAllGather")) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (lib) {
            a.AllGather = (decltype(a.AllGather))dlsym(lib, "ncclAllGather");
            a.Send = (decltype(a.Send))dlsym(lib, "ncclSend");
            a.Recv = (decltype(a.Recv))dlsym(lib, "ncclRecv");
            a.GroupStart = (decltype(a.GroupStart))dlsym(lib, "ncclGroupStart");
            a.GroupEnd = (decltype(a.GroupEnd))dlsym(lib, "ncclGroupEnd");
            a.ok = a.AllGather && a.Send && a.Recv && a.GroupStart && a.GroupEnd;
        }
        return a;
    }();
    return api;
}
enum { kNcclUint8 = 1, kNcclUint64 = 5 };  // ncclDataType_t (rccl.h)

// every rank's slice of `gathered` to every peer: one grouped batch of sends and receives, so that
// each of a GPU's xGMI links carries one peer's shard (no ring)
int exchange_slices(flate_hip_ctx* h, void* comm, int rank, int world, uint8_t* gathered, uint64_t slice_bytes,
                    uint64_t send_bytes) {
    const RcclApi& r = rccl();
    if (world == 1) return FLATE_HIP_OK;
    if (r.GroupStart() != 0) return FLATE_HIP_E_LAUNCH;
    for (int d = 1; d < world; d++) {
        const int to = (rank + d) % world, from = (rank - d + world) % world;
        if (r.Send(gathered + (uint64_t)rank * slice_bytes, send_bytes, kNcclUint8, to, comm, h->stream) != 0 ||
            r.Recv(gathered + (uint64_t)from * slice_bytes, send_bytes, kNcclUint8, from, comm, h->stream) != 0) {
            (void)r.GroupEnd();
            h->last_error = "ncclSend / ncclRecv failed";
            return FLATE_HIP_E_LAUNCH;
        }
    }
    if (r.GroupEnd() != 0) {
        h->last_error = "ncclGroupEnd failed";
        return FLATE_HIP_E_LAUNCH;
    }
    return FLATE_HIP_OK;
}
}  // namespace

int flate_hip_compress_batch_sharded(flate_hip_handle h, void* nccl_comm, int rank, int world, const uint8_t* in,
                                     const uint64_t* in_off, uint32_t n_chunks, int container, int mode, uint8_t* out,
                                     const uint64_t* out_off, uint64_t* out_len, int32_t* status, uint8_t* gathered,
                                     uint64_t slice_bytes, uint64_t* sizes, uint64_t* dst_off) {
    if (!h || !nccl_comm || world <= 0 || rank < 0 || rank >= world || !gathered || !sizes || !dst_off)
        return FLATE_HIP_E_INVALID_ARG;
    if (!rccl().ok) {
        h->last_error = "RCCL (librccl.so) not available";
        return FLATE_HIP_E_UNSUPPORTED;
    }
    const bool was_sync = h->sync;
    h->sync = false;  // everything below is ordered on the handle's stream
    int rc = compress_impl(h, in, in_off, n_chunks, container, mode, out, out_off, out_len, status,
                           FLATE_HIP_MEM_DEVICE, nullptr);
    // this rank's streams back to back at the head of its slice; dst_off[n_chunks] = packed size
    if (!rc) rc = flate_hip_gather_streams(h, out, out_off, out_len, n_chunks, gathered + (uint64_t)rank * slice_bytes, dst_off);
    if (!rc && rccl().AllGather(dst_off + n_chunks, sizes, 1, kNcclUint64, nccl_comm, h->stream) != 0) {
        h->last_error = "ncclAllGather failed";
        rc = FLATE_HIP_E_LAUNCH;
    }
    // every peer gets the largest packed shard's worth of bytes, not the slice's capacity (the sizes are read once:
    // one wait on the stream; a caller needs them anyway to use gathered[])
    uint64_t send_bytes = slice_bytes;
    if (!rc && world > 1) {
        std::vector<uint64_t> hs((size_t)world);
        if (hipMemcpyAsync(hs.data(), sizes, sizeof(uint64_t) * (size_t)world, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            h->last_error = "reading the packed sizes failed";
            rc = FLATE_HIP_E_LAUNCH;
        } else {
            uint64_t mx = 0;
            for (uint64_t v : hs) mx = std::max(mx, v);
            if (mx > slice_bytes) {
                h->last_error = "a packed shard is larger than slice_bytes";
                rc = FLATE_HIP_E_INVALID_ARG;
            } else {
                send_bytes = std::min<uint64_t>(slice_bytes, (mx + 15) & ~(uint64_t)15);
            }
        }
    }
    if (!rc) rc = exchange_slices(h, nccl_comm, rank, world, gathered, slice_bytes, send_bytes);
    h->sync = was_sync;
    if (!rc && h->sync) HIP_OK(h, hipStreamSynchronize(h->stream));
    return rc;
}

int flate_hip_decompress_batch_sharded(flate_hip_handle h, void* nccl_comm, int rank, int world, const uint8_t* in,
                                       const uint64_t* in_off, uint32_t n_chunks, int container, int flags,
                                       uint8_t* gathered, uint64_t slice_bytes, const uint64_t* out_off,
                                       uint64_t* out_len, int32_t* status, uint64_t* consumed) {
    if (!h || !nccl_comm || world <= 0 || rank < 0 || rank >= world || !gathered) return FLATE_HIP_E_INVALID_ARG;
    if (!rccl().ok) {
        h->last_error = "RCCL (librccl.so) not available";
        return FLATE_HIP_E_UNSUPPORTED;
    }
    const bool was_sync = h->sync;
    h->sync = false;
    // the outputs of this rank's streams go straight into its slice (out_off is relative to the slice)
    int rc = flate_hip_decompress_batch(h, in, in_off, n_chunks, container, flags, gathered + (uint64_t)rank * slice_bytes,
                                        out_off, out_len, status, consumed, FLATE_HIP_MEM_DEVICE);
    // every peer gets what the fullest slice holds (the end of its last slot), not the slices' capacity: the ends are
    // all-gathered and read once (one wait on the stream; decompress has waited for its offsets already)
    uint64_t send_bytes = slice_bytes;
    if (!rc && world > 1) {
        std::vector<uint64_t> hs((size_t)world + 1, 0);
        if ((rc = ensure(h, h->shard_sz, sizeof(uint64_t) * ((size_t)world + 1))) == 0) {
            uint64_t* dsz = (uint64_t*)h->shard_sz.p;
            if (hipMemcpyAsync(dsz + world, out_off + n_chunks, sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream) != hipSuccess ||
                rccl().AllGather(dsz + world, dsz, 1, kNcclUint64, nccl_comm, h->stream) != 0 ||
                hipMemcpyAsync(hs.data(), dsz, sizeof(uint64_t) * (size_t)world, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess) {
                h->last_error = "exchanging the slice sizes failed";
                rc = FLATE_HIP_E_LAUNCH;
            } else {
                uint64_t mx = 0;
                for (int i = 0; i < world; i++) mx = std::max(mx, hs[(size_t)i]);
                if (mx > slice_bytes) {
                    h->last_error = "a rank's slots end beyond slice_bytes";
                    rc = FLATE_HIP_E_INVALID_ARG;
                } else {
                    send_bytes = std::min<uint64_t>(slice_bytes, (mx + 15) & ~(uint64_t)15);
                }
            }
        }
    }
    if (!rc) rc = exchange_slices(h, nccl_comm, rank, world, gathered, slice_bytes, send_bytes);
    h->sync = was_sync;
    if (!rc && h->sync) HIP_OK(h, hipStreamSynchronize(h->stream));
    return rc;
}

int flate_hip_plan_compress(flate_hip_handle h, const uint64_t* in_off, const uint64_t* out_off, uint32_t n_chunks,
                            int container, int mode, flate_hip_plan_t* plan) {
    if (!h || !in_off || !out_off || !plan || n_chunks == 0) return FLATE_HIP_E_INVALID_ARG;
    *plan = nullptr;
    flate_hip_plan* pl = new flate_hip_plan();
    pl->hin.assign(in_off, in_off + n_chunks + 1);
    pl->hout.assign(out_off, out_off + n_chunks + 1);
    pl->n_chunks = n_chunks;
    pl->container = container;
    pl->mode = mode;
    for (uint32_t i = 0; i < n_chunks; i++)
        if (pl->hin[i + 1] < pl->hin[i] || pl->hout[i + 1] < pl->hout[i]) {
            delete pl;
            return FLATE_HIP_E_INVALID_ARG;
        }
    const int rc = compress_impl(h, nullptr, nullptr, n_chunks, container, mode, nullptr, nullptr, nullptr, nullptr,
                                 FLATE_HIP_MEM_DEVICE, nullptr, pl);
    if (rc) {
        (void)flate_hip_plan_destroy(h, pl);
        return rc;
    }
    pl->ready = true;
    *plan = pl;
    return FLATE_HIP_OK;
}

int flate_hip_compress_planned(flate_hip_handle h, flate_hip_plan_t plan, const uint8_t* in, uint8_t* out,
                               uint64_t* out_len, int32_t* status) {
    if (!h || !plan || !plan->ready || !in || !out) return FLATE_HIP_E_INVALID_ARG;
    return compress_impl(h, in, nullptr, plan->n_chunks, plan->container, plan->mode, out, nullptr, out_len, status,
                         FLATE_HIP_MEM_DEVICE, nullptr, plan);
}

int flate_hip_plan_destroy(flate_hip_handle h, flate_hip_plan_t plan) {
    if (!h || !plan) return FLATE_HIP_E_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (auto& pp : plan->passes) {
        if (pp.chunks) (void)hipFree(pp.chunks);
        if (pp.blk_chunk) (void)hipFree(pp.blk_chunk);
    }
    delete plan;
    return FLATE_HIP_OK;
}

int flate_hip_checksum(flate_hip_handle h, const uint8_t* data, uint64_t n, int container, uint32_t* value) {
    if (!h || !value || (n && !data) || (container != 1 && container != 2) || n > 0xfffffff0ull) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    int rc;
    // one huffman-only style chunk: block j = bytes [65535 j, ...)
    fl_chunk ck{};
    ck.in_len = (uint32_t)n;
    ck.n_blocks = (uint32_t)(n / FL_BLOCK_BYTES + 1);
    const uint32_t nb = ck.n_blocks;
    std::vector<uint32_t> blk_chunk(nb, 0u);
    fl_params prm{};
    prm.n_chunks = 1;
    prm.n_blocks = nb;
    prm.container = container;
    prm.mode = 1;
    if ((rc = ensure(h, h->chunks, sizeof(fl_chunk)))) return rc;
    if ((rc = ensure(h, h->blk_chunk, sizeof(uint32_t) * nb))) return rc;
    if ((rc = ensure(h, h->cks, sizeof(uint32_t) * 2 * (size_t)nb + 16))) return rc;
    if ((rc = ensure(h, h->st_in, n + 16))) return rc;
    if ((rc = ensure(h, h->st_status, 16))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->chunks.p, &ck, sizeof ck, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->blk_chunk.p, blk_chunk.data(), sizeof(uint32_t) * nb, hipMemcpyHostToDevice, st));
    if (n) HIP_OK(h, hipMemcpyAsync(h->st_in.p, data, n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_checksum, dim3(nb), dim3(64), 0, st, (const uint8_t*)h->st_in.p, (const fl_chunk*)h->chunks.p,
                       (const uint32_t*)h->blk_chunk.p, (const fl_sblock*)nullptr, prm, h->crc, (uint32_t*)h->cks.p);
    hipLaunchKernelGGL(k_fold_checksum, dim3(1), dim3(64), 0, st, (const uint32_t*)h->cks.p, nb, container, h->crc,
                       (uint32_t*)h->st_status.p);
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, hipMemcpyAsync(value, h->st_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    return FLATE_HIP_OK;
}

uint32_t flate_hip_checksum_combine(int container, uint32_t a, uint32_t b, uint64_t len_b) {
    if (container == 1) {
        // crc(A || B) = crc(A) * x^(8 |B|) + crc(B) in the reflected representation (as zlib's crc32_combine)
        fl_crc_consts cc;
        init_crc_consts(cc);
        return fl_crc_mulmod(a, fl_crc_xpow8n(cc.xpow8, len_b)) ^ b;
    }
    // Adler-32: a = a1 + a2 - 1, b = b1 + b2 + |B| (a1 - 1)   (mod 65521)
    const uint32_t a1 = a & 0xffff, b1 = a >> 16, a2 = b & 0xffff, b2 = b >> 16;
    const uint32_t rem = (uint32_t)(len_b % 65521u);
    const uint32_t an = (a1 + a2 + 65521u - 1u) % 65521u;
    const uint32_t bn = (uint32_t)(((uint64_t)b1 + b2 + (uint64_t)rem * ((a1 + 65521u - 1u) % 65521u)) % 65521u);
    return an | (bn << 16);
}

}  // extern "C"

// ---- resumable inflate (kernels_inflate.h, k_inflater) ----
struct flate_hip_inflater {
    uint32_t n = 0;
    int container = 0, flags = 0;
    void* sess = nullptr;  // FL_RS_STRIDE bytes per stream: state, carry, input window, history, output window
    // host-memory feeds: the pieces, offsets and slots on the device
    DevBuf in, in_off, fin, out, out_off, out_len, consumed, status, which;
    DevBuf dict, dict_tab, applied;  // flate_hip_inflater_set_dictionary: a host caller's dictionary, its table entry, the answers
    bool dict_aware = false;  // feeds run k_inflater_dict: created with FLATE_HIP_INFLATER_NEED_DICT, or a dictionary was ever set
    std::vector<uint8_t> host_out;  // host-memory feeds of many streams: the slots on their way to the caller
};

namespace {
// ---- the device buffers of the resumable sessions (inflaters, deflaters): they only grow, with room to spare, and
// belong to the session, not to the handle's workspace.  `who` owns the buffer ("an inflater": the error text); `held`,
// where given, counts the bytes (the deflaters': flate_hip_debug_device_bytes).
void session_free(DevBuf& b, uint64_t* held = nullptr) {
    if (b.p) {
        (void)hipFree(b.p);
        if (held) *held -= b.cap;
    }
    b = DevBuf();
}
int session_grow(flate_hip_ctx* h, DevBuf& b, size_t bytes, const char* who, uint64_t* held = nullptr) {
    if (bytes <= b.cap) return FLATE_HIP_OK;
    (void)hipStreamSynchronize(h->stream);
    session_free(b, held);
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        h->last_error = "hipMalloc(" + std::to_string(want) + ") for " + who + " feed failed";
        return FLATE_HIP_E_ALLOC;
    }
    b.cap = want;
    if (held) *held += want;
    return FLATE_HIP_OK;
}

int inflater_reset_all(flate_hip_ctx* h, flate_hip_inflater* s, const uint32_t* d_which, uint32_t n) {
    if (n == 0) return FLATE_HIP_OK;
    hipLaunchKernelGGL(k_inflater_reset, dim3((n + 255) / 256), dim3(256), 0, h->stream, (uint8_t*)s->sess, d_which, n, s->n,
                       s->container);
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// one launch for both memory kinds: the kernel reads the offsets, flags and slots where they lie
int launch_inflater(flate_hip_ctx* h, flate_hip_inflater* s, const uint8_t* in, const uint64_t* in_off, const uint8_t* final_,
                    uint8_t* out, const uint64_t* out_off, uint64_t* out_len, uint64_t* consumed, int32_t* status) {
    ProfScope ps(h, K_INFLATER);
    hipLaunchKernelGGL(s->dict_aware ? k_inflater_dict : k_inflater, dim3(s->n), dim3(64), 0, h->stream, in, in_off, final_, out,
                       out_off, out_len, consumed, status, (uint8_t*)s->sess, s->container, s->flags, h->crc);
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// ---- a host-memory feed runs on copies (the rules: inflate_plan.h).  The pieces, the offsets from 0 and the flags go to the
// device ...
int stage_inflater_feed(flate_hip_ctx* h, flate_hip_inflater* s, const uint8_t* in, uint64_t in_lo, const uint8_t* final_,
                        const std::vector<uint64_t>& hin, const std::vector<uint64_t>& hout) {
    const size_t n = s->n;
    const auto grow = [&](DevBuf& b, size_t bytes) { return session_grow(h, b, bytes, "an inflater"); };
    int rc;
    if ((rc = grow(s->in, hin[n] + 16)) || (rc = grow(s->out, hout[n] + 16)) || (rc = grow(s->in_off, 8 * (n + 1))) ||
        (rc = grow(s->out_off, 8 * (n + 1))) || (rc = grow(s->fin, n)) || (rc = grow(s->out_len, 8 * n)) ||
        (rc = grow(s->consumed, 8 * n)) || (rc = grow(s->status, 4 * n)))
        return rc;
    if (hin[n]) HIP_OK(h, hipMemcpyAsync(s->in.p, in + in_lo, hin[n], hipMemcpyHostToDevice, h->stream));
    HIP_OK(h, hipMemcpyAsync(s->in_off.p, hin.data(), 8 * (n + 1), hipMemcpyHostToDevice, h->stream));
    HIP_OK(h, hipMemcpyAsync(s->out_off.p, hout.data(), 8 * (n + 1), hipMemcpyHostToDevice, h->stream));
    HIP_OK(h, hipMemcpyAsync(s->fin.p, final_, n, hipMemcpyHostToDevice, h->stream));
    return FLATE_HIP_OK;
}

// ... and the results come home, then the produced bytes into the caller's slots (fl_inflater_copy_each)
int inflater_feed_home(flate_hip_ctx* h, flate_hip_inflater* s, const std::vector<uint64_t>& hout, uint8_t* out,
                       const uint64_t* out_off, uint64_t* out_len, uint64_t* consumed, int32_t* status) {
    const uint32_t n = s->n;
    hipStream_t st = h->stream;
    HIP_OK(h, hipMemcpyAsync(out_len, s->out_len.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(consumed, s->consumed.p, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(status, s->status.p, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    if (fl_inflater_copy_each(n)) {
        for (uint32_t i = 0; i < n; i++)
            if (out_len[i]) HIP_OK(h, hipMemcpyAsync(out + out_off[i], (uint8_t*)s->out.p + hout[i], out_len[i], hipMemcpyDeviceToHost, st));
    } else if (hout[n]) {
        s->host_out.resize(hout[n]);
        HIP_OK(h, hipMemcpyAsync(s->host_out.data(), s->out.p, hout[n], hipMemcpyDeviceToHost, st));
        HIP_OK(h, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < n; i++)
            if (out_len[i]) std::memcpy(out + out_off[i], s->host_out.data() + hout[i], out_len[i]);
    }
    HIP_OK(h, hipStreamSynchronize(st));
    return FLATE_HIP_OK;
}
}  // namespace

extern "C" {

int flate_hip_inflater_create(flate_hip_handle h, uint32_t n_streams, int container, int flags, flate_hip_inflater_t* out) {
    if (!h || !out || n_streams == 0 || container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    *out = nullptr;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    flate_hip_inflater* s = new flate_hip_inflater();
    s->n = n_streams;
    s->container = container;
    s->flags = flags & (FLATE_HIP_INFLATE_STRICT_Q6 | (container != FLATE_HIP_GZIP ? FLATE_HIP_INFLATER_NEED_DICT : 0));
    s->dict_aware = (s->flags & FLATE_HIP_INFLATER_NEED_DICT) != 0;
    if (hipMalloc(&s->sess, (size_t)n_streams * FL_RS_STRIDE) != hipSuccess) {
        h->last_error = "hipMalloc of the inflater's state (" + std::to_string((size_t)n_streams * FL_RS_STRIDE) + " bytes) failed";
        delete s;
        return FLATE_HIP_E_ALLOC;
    }
    int rc = inflater_reset_all(h, s, nullptr, n_streams);
    if (rc == FLATE_HIP_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = FLATE_HIP_E_LAUNCH;
    if (rc) {
        (void)hipFree(s->sess);
        delete s;
        return rc;
    }
    *out = s;
    return FLATE_HIP_OK;
}

int flate_hip_inflater_destroy(flate_hip_handle h, flate_hip_inflater_t s) {
    if (!h || !s) return FLATE_HIP_E_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (DevBuf* b : {&s->in, &s->in_off, &s->fin, &s->out, &s->out_off, &s->out_len, &s->consumed, &s->status, &s->which,
                      &s->dict, &s->dict_tab, &s->applied})
        session_free(*b);
    (void)hipFree(s->sess);
    delete s;
    return FLATE_HIP_OK;
}

int flate_hip_inflater_reset(flate_hip_handle h, flate_hip_inflater_t s, const uint32_t* which, uint32_t n_which) {
    if (!h || !s || (n_which && !which)) return FLATE_HIP_E_INVALID_ARG;
    for (uint32_t k = 0; k < n_which; k++)
        if (which[k] >= s->n) return FLATE_HIP_E_INVALID_ARG;
    if (n_which == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    int rc = session_grow(h, s->which, sizeof(uint32_t) * n_which, "an inflater");
    if (rc) return rc;
    // (a pageable source: the copy has been taken when hipMemcpyAsync returns, the kernel is ordered behind it)
    HIP_OK(h, hipMemcpyAsync(s->which.p, which, sizeof(uint32_t) * n_which, hipMemcpyHostToDevice, h->stream));
    if ((rc = inflater_reset_all(h, s, (const uint32_t*)s->which.p, n_which))) return rc;
    if (h->sync) HIP_OK(h, hipStreamSynchronize(h->stream));
    return FLATE_HIP_OK;
}

int flate_hip_inflater_set_dictionary(flate_hip_handle h, flate_hip_inflater_t s, const uint32_t* which, uint32_t n_which,
                                      const uint8_t* dict, uint64_t dict_len, int memkind, uint8_t* applied) {
    if (!h || !s || (n_which && !which) || (dict_len && !dict)) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (s->container == FLATE_HIP_GZIP) return FLATE_HIP_E_INVALID_ARG;
    for (uint32_t k = 0; k < n_which; k++)
        if (which[k] >= s->n) return FLATE_HIP_E_INVALID_ARG;
    if (n_which == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    const auto grow = [&](DevBuf& b, size_t bytes) { return session_grow(h, b, bytes, "an inflater"); };
    int rc;
    if ((rc = grow(s->which, sizeof(uint32_t) * n_which)) || (rc = grow(s->applied, n_which)) || (rc = grow(s->dict_tab, sizeof(fl_dict_ent))))
        return rc;
    const uint8_t* d_dict = dict;
    if (memkind == FLATE_HIP_MEM_HOST) {
        if ((rc = grow(s->dict, dict_len + 16))) return rc;
        if (dict_len) HIP_OK(h, hipMemcpyAsync(s->dict.p, dict, dict_len, hipMemcpyHostToDevice, st));
        d_dict = (const uint8_t*)s->dict.p;
    }
    const uint64_t off[2] = {0, dict_len};
    std::vector<fl_dict_ent> tab;
    fl_dict_table(off, 1, tab);
    HIP_OK(h, hipMemcpyAsync(s->which.p, which, sizeof(uint32_t) * n_which, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(s->dict_tab.p, tab.data(), sizeof(fl_dict_ent), hipMemcpyHostToDevice, st));
    s->dict_aware = true;
    hipLaunchKernelGGL(k_dict_adler, dim3(1), dim3(64), 0, st, d_dict, (fl_dict_ent*)s->dict_tab.p, 1u);
    hipLaunchKernelGGL(k_inflater_set_dict, dim3(n_which), dim3(64), 0, st, (uint8_t*)s->sess, (const uint32_t*)s->which.p, n_which,
                       s->n, s->container, d_dict, (const fl_dict_ent*)s->dict_tab.p, (uint8_t*)s->applied.p);
    HIP_OK(h, hipGetLastError());
    if (applied) HIP_OK(h, hipMemcpyAsync(applied, s->applied.p, n_which, hipMemcpyDeviceToHost, st));
    // `which` and the table are pageable host memory: their copies have been taken when hipMemcpyAsync returns, and the
    // kernels are ordered behind them (as in flate_hip_inflater_reset), so nothing here has to wait for them.  A host
    // caller's dictionary may be pinned, so the call waits for its copy; a device caller's dictionary is read in stream
    // order, and without `applied` and with set_sync(0) the call returns before that.
    if (applied || memkind == FLATE_HIP_MEM_HOST || h->sync) HIP_OK(h, hipStreamSynchronize(st));
    return FLATE_HIP_OK;
}

int flate_hip_inflater_feed(flate_hip_handle h, flate_hip_inflater_t s, const uint8_t* in, const uint64_t* in_off,
                            const uint8_t* final_, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                            uint64_t* consumed, int32_t* status, int memkind) {
    if (!h || !s || !in_off || !final_ || !out_off || !out_len || !consumed || !status) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    int rc;
    if (memkind == FLATE_HIP_MEM_DEVICE) {  // enqueue only: the kernel reads the caller's offsets itself
        if ((rc = launch_inflater(h, s, in, in_off, final_, out, out_off, out_len, consumed, status))) return rc;
        if (h->sync) HIP_OK(h, hipStreamSynchronize(h->stream));
        return FLATE_HIP_OK;
    }
    if (!fl_inflater_slots_ok(in_off, out_off, final_, s->n)) return FLATE_HIP_E_INVALID_ARG;
    std::vector<uint64_t> hin, hout;
    fl_inflater_rebase(in_off, out_off, s->n, hin, hout);
    if ((rc = stage_inflater_feed(h, s, in, in_off[0], final_, hin, hout))) return rc;
    if ((rc = launch_inflater(h, s, (const uint8_t*)s->in.p, (const uint64_t*)s->in_off.p, (const uint8_t*)s->fin.p, (uint8_t*)s->out.p,
                              (const uint64_t*)s->out_off.p, (uint64_t*)s->out_len.p, (uint64_t*)s->consumed.p, (int32_t*)s->status.p)))
        return rc;
    return inflater_feed_home(h, s, hout, out, out_off, out_len, consumed, status);
}

}  // extern "C"

// ---- resumable compress, huffman-only / store-only (kernels_deflater.h) ----
struct flate_hip_deflater {
    uint32_t n = 0;
    int container = 0, mode = 0;
    DevBuf state, bufs;  // fl_dfl_state and FL_DFL_BUF bytes of SimpleCompressor buffer per stream
    std::vector<fl_dfl_mirror> mirror;  // per stream: the counters the feeds plan with (deflater_plan.h) ...
    std::vector<DevBuf> pend;           // ... and the bytes of its pending output
    // feed workspace: the pieces (host feeds), the staged input, the produced blocks, the tables
    DevBuf src, win, wout, chunks, blk, sb, ckblk, cksb, jobs, produced, plans, hist, cks;
};

static_assert((int)FL_FEED_MORE == (int)FLATE_HIP_FEED_MORE && (int)FL_FEED_FLUSH == (int)FLATE_HIP_FEED_FLUSH &&
                  (int)FL_FEED_FINISH == (int)FLATE_HIP_FEED_FINISH && (int)FL_DFL_ST_OK == (int)FLATE_HIP_ST_OK &&
                  (int)FL_DFL_ST_NEED_INPUT == (int)FLATE_HIP_ST_NEED_INPUT && (int)FL_DFL_ST_NEED_OUTPUT == (int)FLATE_HIP_ST_NEED_OUTPUT,
              "deflater_plan.h speaks of the ops and statuses of include/flate_hip.h");

namespace {

// ---- flate_hip_deflater_feed: what a feed decides is deflater_plan.h's, the stages below carry it out over one record
// per call.  (A feed that fails halfway -- an allocation for pending output, a HIP call -- leaves the mirror moved on for
// the streams it had settled or drained by then.)
struct DeflaterFeed {
    flate_hip_ctx* h;
    flate_hip_deflater* d;
    hipStream_t st;
    const uint8_t* in;  // the caller's buffers
    uint8_t* out;
    bool dev;                         // device memory
    std::vector<uint64_t> hin, hout;  // the caller's tables on the host
    std::vector<uint8_t> hop;
    std::vector<uint64_t> r_len, r_cons;  // what the feed answers
    std::vector<int32_t> r_st;
    std::vector<uint32_t> act;  // the streams that take their piece: job j is stream act[j]
    fl_dfl_layout lay;
    fl_params prm{};
    const uint8_t* src = nullptr;  // where the jobs' src_off count from: the caller's buffer, or the staged pieces

    hipMemcpyKind to_out() const { return dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
    int grow(DevBuf& b, size_t bytes) { return session_grow(h, b, bytes, "a deflater", &h->dfl_bytes); }
};

// offsets and ops on the host: the block tables are built here (device feeds wait for them)
int fetch_feed_tables(DeflaterFeed& df, const uint64_t* in_off, const uint64_t* out_off, const uint8_t* op) {
    flate_hip_ctx* h = df.h;
    const size_t n = df.d->n;
    df.hin.resize(n + 1);
    df.hout.resize(n + 1);
    df.hop.resize(n);
    if (df.dev) {
        HIP_OK(h, hipMemcpyAsync(df.hin.data(), in_off, 8 * (n + 1), hipMemcpyDeviceToHost, df.st));
        HIP_OK(h, hipMemcpyAsync(df.hout.data(), out_off, 8 * (n + 1), hipMemcpyDeviceToHost, df.st));
        HIP_OK(h, hipMemcpyAsync(df.hop.data(), op, n, hipMemcpyDeviceToHost, df.st));
        HIP_OK(h, hipStreamSynchronize(df.st));
    } else {
        std::memcpy(df.hin.data(), in_off, 8 * (n + 1));
        std::memcpy(df.hout.data(), out_off, 8 * (n + 1));
        std::memcpy(df.hop.data(), op, n);
    }
    return FLATE_HIP_OK;
}

// every stream's route (fl_dfl_route_stream); pending output goes into the slots here
int drain_and_route(DeflaterFeed& df) {
    flate_hip_ctx* h = df.h;
    flate_hip_deflater* d = df.d;
    df.r_len.assign(d->n, 0);
    df.r_cons.assign(d->n, 0);
    df.r_st.assign(d->n, FLATE_HIP_ST_NEED_INPUT);
    for (uint32_t i = 0; i < d->n; i++) {
        const fl_dfl_route r = fl_dfl_route_stream(d->mirror[i], df.hin[i + 1] - df.hin[i], df.hop[i], df.hout[i + 1] - df.hout[i]);
        if (r.give) HIP_OK(h, hipMemcpyAsync(df.out + df.hout[i], (const uint8_t*)d->pend[i].p + r.from, r.give, df.to_out(), df.st));
        df.r_len[i] = r.give;
        df.r_st[i] = r.status;
        if (r.kind == FL_DFL_ACTIVE) df.act.push_back(i);
    }
    return FLATE_HIP_OK;
}

void lay_out_feed(DeflaterFeed& df) {
    const flate_hip_deflater* d = df.d;
    fl_dfl_lay_out(d->mirror.data(), df.act, df.hin.data(), df.hop.data(), df.dev, df.lay);
    (void)level_args(d->mode, df.prm);
    df.prm.container = d->container;
    df.prm.mode = d->mode;
    df.prm.n_chunks = (uint32_t)df.act.size();
    df.prm.n_blocks = (uint32_t)df.lay.blocks.size();
}

int reserve_feed_buffers(DeflaterFeed& df) {
    flate_hip_deflater* d = df.d;
    const fl_dfl_layout& lay = df.lay;
    const size_t nj = lay.jobs.size(), nb = std::max<size_t>(lay.blocks.size(), 1), nck = std::max<size_t>(lay.units.size(), 1);
    int rc;
    if ((!df.dev && (rc = df.grow(d->src, df.hin[d->n] - df.hin[0] + 16))) || (rc = df.grow(d->win, lay.win_n + 16)) || (rc = df.grow(d->wout, lay.out_n + 16)) ||
        (rc = df.grow(d->jobs, sizeof(fl_dfl_job) * nj)) || (rc = df.grow(d->chunks, sizeof(fl_chunk) * nj)) ||
        (rc = df.grow(d->produced, 8 * nj)) || (rc = df.grow(d->blk, 4 * nb)) || (rc = df.grow(d->sb, sizeof(fl_sblock) * nb)) ||
        (rc = df.grow(d->ckblk, 4 * nck)) || (rc = df.grow(d->cksb, sizeof(fl_sblock) * nck)) ||
        (rc = df.grow(d->plans, sizeof(fl_block_plan) * nb)) || (rc = df.grow(d->hist, 4 * 320 * nb)) || (rc = df.grow(d->cks, 8 * nck)))
        return rc;
    return FLATE_HIP_OK;
}

// a host feed's pieces, the tables, and a cleared output (the bit packer ORs into it)
int upload_feed_tables(DeflaterFeed& df) {
    flate_hip_ctx* h = df.h;
    flate_hip_deflater* d = df.d;
    const fl_dfl_layout& lay = df.lay;
    const size_t nj = lay.jobs.size(), nb = lay.blocks.size(), nck = lay.units.size();
    const uint64_t in_lo = df.hin[0], in_hi = df.hin[d->n];
    df.src = df.in;
    if (!df.dev) {
        if (in_hi > in_lo) HIP_OK(h, hipMemcpyAsync(d->src.p, df.in + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, df.st));
        df.src = (const uint8_t*)d->src.p;
    }
    HIP_OK(h, hipMemcpyAsync(d->jobs.p, lay.jobs.data(), sizeof(fl_dfl_job) * nj, hipMemcpyHostToDevice, df.st));
    HIP_OK(h, hipMemcpyAsync(d->chunks.p, lay.chunks.data(), sizeof(fl_chunk) * nj, hipMemcpyHostToDevice, df.st));
    if (nb) {
        HIP_OK(h, hipMemcpyAsync(d->blk.p, lay.block_job.data(), 4 * nb, hipMemcpyHostToDevice, df.st));
        HIP_OK(h, hipMemcpyAsync(d->sb.p, lay.blocks.data(), sizeof(fl_sblock) * nb, hipMemcpyHostToDevice, df.st));
    }
    if (nck) {
        HIP_OK(h, hipMemcpyAsync(d->ckblk.p, lay.unit_job.data(), 4 * nck, hipMemcpyHostToDevice, df.st));
        HIP_OK(h, hipMemcpyAsync(d->cksb.p, lay.units.data(), sizeof(fl_sblock) * nck, hipMemcpyHostToDevice, df.st));
    }
    HIP_OK(h, hipMemsetAsync(d->wout.p, 0, lay.out_n, df.st));
    return FLATE_HIP_OK;
}

// stage, checksum, plan, place (k_deflater_offsets), pack, keep (k_deflater_commit)
int enqueue_feed_kernels(DeflaterFeed& df) {
    flate_hip_ctx* h = df.h;
    flate_hip_deflater* d = df.d;
    hipStream_t st = df.st;
    const uint32_t nj = (uint32_t)df.lay.jobs.size(), nb = (uint32_t)df.lay.blocks.size(), nck = (uint32_t)df.lay.units.size();
    const fl_dfl_job* djobs = (const fl_dfl_job*)d->jobs.p;
    const fl_chunk* dch = (const fl_chunk*)d->chunks.p;
    const uint32_t* dblk = (const uint32_t*)d->blk.p;
    const fl_sblock* dsb = (const fl_sblock*)d->sb.p;
    fl_block_plan* dpl = (fl_block_plan*)d->plans.p;
    const uint8_t* dwin = (const uint8_t*)d->win.p;
    {
        ProfScope ps(h, K_DEFLATER);
        hipLaunchKernelGGL(k_deflater_stage, dim3(nj, df.lay.slices), dim3(256), 0, st, df.src, djobs, dch, (const uint8_t*)d->bufs.p,
                           (uint8_t*)d->win.p);
    }
    if (d->container != 0 && nck) {
        ProfScope ps(h, K_CHECKSUM);
        hipLaunchKernelGGL(k_checksum, dim3(nck), dim3(64), 0, st, dwin, dch, (const uint32_t*)d->ckblk.p,
                           (const fl_sblock*)d->cksb.p, df.prm, h->crc, (uint32_t*)d->cks.p);
    }
    if (nb) {
        ProfScope ps(h, K_PLAN);
        if (d->mode == 0) {
            hipLaunchKernelGGL(k_plan_store, dim3((nb + 255) / 256), dim3(256), 0, st, dch, dblk, dsb, nb, dpl);
        } else {
            hipLaunchKernelGGL(k_byte_hist, dim3(nb), dim3(256), 0, st, dwin, dch, dblk, dsb, (uint32_t*)d->hist.p);
            hipLaunchKernelGGL(k_plan, dim3((nb + FL_PLAN_WAVES - 1) / FL_PLAN_WAVES), dim3(64 * FL_PLAN_WAVES), 0, st,
                               dch, dblk, dsb, df.prm, (const uint32_t*)d->hist.p, dpl);
        }
    }
    {
        ProfScope ps(h, K_DEFLATER);
        hipLaunchKernelGGL(k_deflater_offsets, dim3(nj), dim3(64), 0, st, djobs, dch, df.prm, h->crc, dpl, (const uint32_t*)d->cks.p,
                           (fl_dfl_state*)d->state.p, (uint8_t*)d->wout.p, (uint64_t*)d->produced.p);
    }
    if (nb) {
        ProfScope ps(h, K_ENCODE);
        hipLaunchKernelGGL(k_encode<false>, dim3(nb), dim3(64 * FL_ENC_WAVES), 0, st, dwin, dch, dblk,
                           (const fl_block_plan*)dpl, (const uint32_t*)nullptr, (uint32_t*)d->wout.p);
    }
    {
        ProfScope ps(h, K_DEFLATER);
        hipLaunchKernelGGL(k_deflater_commit, dim3(nj), dim3(256), 0, st, djobs, dch, (const uint64_t*)d->produced.p, dwin,
                           (const uint8_t*)d->wout.p, (fl_dfl_state*)d->state.p, (uint8_t*)d->bufs.p);
    }
    HIP_OK(h, hipGetLastError());
    return FLATE_HIP_OK;
}

// every job's produced bytes: into the slot, the rest kept as pending output (fl_dfl_settle)
int settle_and_deliver(DeflaterFeed& df) {
    flate_hip_ctx* h = df.h;
    flate_hip_deflater* d = df.d;
    const uint32_t nj = (uint32_t)df.lay.jobs.size();
    std::vector<uint64_t> prod(nj);
    HIP_OK(h, hipMemcpyAsync(prod.data(), d->produced.p, 8 * (size_t)nj, hipMemcpyDeviceToHost, df.st));
    HIP_OK(h, hipStreamSynchronize(df.st));
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = df.act[j];
        const fl_chunk& ck = df.lay.chunks[j];
        fl_dfl_mirror m = d->mirror[i];
        const fl_dfl_settled s = fl_dfl_settle(m, df.lay.jobs[j], ck, prod[j], df.hout[i + 1] - df.hout[i]);
        if (!s.ok) {
            h->last_error = "deflater feed: a stream produced more than its bound";
            return FLATE_HIP_E_LAUNCH;
        }
        const uint8_t* from = (const uint8_t*)d->wout.p + ck.out_off;
        if (s.give) HIP_OK(h, hipMemcpyAsync(df.out + df.hout[i], from, s.give, df.to_out(), df.st));
        if (s.pend) {
            if (int rc = df.grow(d->pend[i], s.pend)) return rc;
            HIP_OK(h, hipMemcpyAsync(d->pend[i].p, from + s.give, s.pend, hipMemcpyDeviceToDevice, df.st));
        }
        d->mirror[i] = m;
        df.r_len[i] = s.give;
        df.r_cons[i] = s.consumed;
        df.r_st[i] = s.status;
    }
    return FLATE_HIP_OK;
}

int feed_results_home(DeflaterFeed& df, uint64_t* out_len, uint64_t* consumed, int32_t* status) {
    flate_hip_ctx* h = df.h;
    const size_t n = df.d->n;
    if (df.dev) {
        HIP_OK(h, hipMemcpyAsync(out_len, df.r_len.data(), 8 * n, hipMemcpyHostToDevice, df.st));
        HIP_OK(h, hipMemcpyAsync(consumed, df.r_cons.data(), 8 * n, hipMemcpyHostToDevice, df.st));
        HIP_OK(h, hipMemcpyAsync(status, df.r_st.data(), 4 * n, hipMemcpyHostToDevice, df.st));
    } else {
        std::memcpy(out_len, df.r_len.data(), 8 * n);
        std::memcpy(consumed, df.r_cons.data(), 8 * n);
        std::memcpy(status, df.r_st.data(), 4 * n);
    }
    HIP_OK(h, hipStreamSynchronize(df.st));
    return FLATE_HIP_OK;
}

}  // namespace

extern "C" {

int flate_hip_deflater_create(flate_hip_handle h, uint32_t n_streams, int container, int mode, uint32_t flags,
                              flate_hip_deflater_t* out) {
    if (!h || !out || n_streams == 0 || container < 0 || container > 2) return FLATE_HIP_E_INVALID_ARG;
    // (FLATE_HIP_DEFLATE_REPAIR_Q1 is the only flag: Q1 is a seam between token blocks, so it never arises in the modes a
    // deflater runs -- nothing to keep)
    if (flags & ~(uint32_t)FLATE_HIP_DEFLATE_REPAIR_Q1) return FLATE_HIP_E_INVALID_ARG;
    *out = nullptr;
    fl_params prm{};
    if (!level_args(mode, prm)) return FLATE_HIP_E_INVALID_ARG;
    if (mode >= 4) {
        h->last_error = "flate_hip_deflater_create: levels 4..9 are not resumable; modes 0 (store) and 1 (huffman) are";
        return FLATE_HIP_E_UNSUPPORTED;
    }
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    flate_hip_deflater* d = new flate_hip_deflater();
    d->n = n_streams;
    d->container = container;
    d->mode = mode;
    d->pend.resize(n_streams);
    d->mirror.assign(n_streams, fl_dfl_mirror());
    int rc = session_grow(h, d->state, sizeof(fl_dfl_state) * (size_t)n_streams, "a deflater", &h->dfl_bytes);
    if (!rc) rc = session_grow(h, d->bufs, (size_t)FL_DFL_BUF * n_streams, "a deflater", &h->dfl_bytes);
    if (!rc && (hipMemsetAsync(d->state.p, 0, sizeof(fl_dfl_state) * (size_t)n_streams, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess))
        rc = FLATE_HIP_E_LAUNCH;
    if (rc) {
        session_free(d->state, &h->dfl_bytes);
        session_free(d->bufs, &h->dfl_bytes);
        delete d;
        return rc;
    }
    *out = d;
    return FLATE_HIP_OK;
}

int flate_hip_deflater_destroy(flate_hip_handle h, flate_hip_deflater_t d) {
    if (!h || !d) return FLATE_HIP_E_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (DevBuf* b : {&d->state, &d->bufs, &d->src, &d->win, &d->wout, &d->chunks, &d->blk, &d->sb, &d->ckblk, &d->cksb,
                      &d->jobs, &d->produced, &d->plans, &d->hist, &d->cks})
        session_free(*b, &h->dfl_bytes);
    for (DevBuf& b : d->pend) session_free(b, &h->dfl_bytes);
    delete d;
    return FLATE_HIP_OK;
}

int flate_hip_deflater_reset(flate_hip_handle h, flate_hip_deflater_t d, const uint32_t* which, uint32_t n_which) {
    if (!h || !d || (n_which && !which)) return FLATE_HIP_E_INVALID_ARG;
    for (uint32_t k = 0; k < n_which; k++)
        if (which[k] >= d->n) return FLATE_HIP_E_INVALID_ARG;
    if (n_which == 0) return FLATE_HIP_OK;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    for (uint32_t k = 0; k < n_which; k++) {
        const uint32_t i = which[k];
        d->mirror[i] = fl_dfl_mirror();
        HIP_OK(h, hipMemsetAsync((fl_dfl_state*)d->state.p + i, 0, sizeof(fl_dfl_state), h->stream));
    }
    HIP_OK(h, hipStreamSynchronize(h->stream));
    return FLATE_HIP_OK;
}

int flate_hip_deflater_feed(flate_hip_handle h, flate_hip_deflater_t d, const uint8_t* in, const uint64_t* in_off,
                            const uint8_t* op, uint8_t* out, const uint64_t* out_off, uint64_t* out_len,
                            uint64_t* consumed, int32_t* status, int memkind) {
    if (!h || !d || !in_off || !op || !out_off || !out_len || !consumed || !status) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    DeflaterFeed df{h, d, h->stream, in, out, memkind == FLATE_HIP_MEM_DEVICE};
    int rc;
    if ((rc = fetch_feed_tables(df, in_off, out_off, op))) return rc;
    if (!fl_dfl_feed_ok(df.hin.data(), df.hout.data(), df.hop.data(), d->n, in != nullptr)) return FLATE_HIP_E_INVALID_ARG;
    if ((rc = drain_and_route(df))) return rc;
    if (!df.act.empty()) {
        lay_out_feed(df);
        if ((rc = reserve_feed_buffers(df))) return rc;
        if ((rc = upload_feed_tables(df))) return rc;
        if ((rc = enqueue_feed_kernels(df))) return rc;
        if ((rc = settle_and_deliver(df))) return rc;
    }
    return feed_results_home(df, out_len, consumed, status);
}

int flate_hip_debug_device_bytes(flate_hip_handle h, uint64_t* bytes) {
    if (!h || !bytes) return FLATE_HIP_E_INVALID_ARG;
    *bytes = h->dfl_bytes;
    return FLATE_HIP_OK;
}

int flate_hip_debug_workspace_bytes(flate_hip_handle h, uint64_t* bytes) {
    if (!h || !bytes) return FLATE_HIP_E_INVALID_ARG;
    // what ensure() holds, less the buffers that hold the batch itself: the staged copies of a host call's data and the
    // batch's chunk and block tables grow with the batch by design, the passes' workspace must not
    uint64_t batch = 0;
    for (const DevBuf* b : {&h->st_in, &h->st_out, &h->st_inoff, &h->st_outlen, &h->st_status, &h->st_consumed, &h->st_pack,
                            &h->st_packoff, &h->st_slot, &h->chunks, &h->blk_chunk})
        batch += b->cap;
    *bytes = h->ws_bytes - batch;
    return FLATE_HIP_OK;
}

int flate_hip_debug_inflate_paths(flate_hip_handle h, uint64_t counts[4]) {
    if (!h || !counts) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    uint32_t handed = 0;
    if (h->dbg_par_taken) {
        HIP_OK(h, hipStreamSynchronize(h->stream));
        HIP_OK(h, hipMemcpy(&handed, h->dbg_par_handed.p, sizeof handed, hipMemcpyDeviceToHost));
    }
    counts[0] = h->dbg_span_done;
    counts[1] = h->dbg_span_taken - h->dbg_span_done;
    counts[2] = h->dbg_par_taken - handed;
    counts[3] = handed;
    return FLATE_HIP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The seek index (index_plan.h, kernels_index.h): its tables live on the host, its windows on the device.
struct flate_hip_index {
    fl_idx_tab tab;
    uint8_t* d_win = nullptr;  // tab.win_bytes bytes
    // made by flate_hip_compress_joined_indexed (or imported from a version-2 blob): every point is a piece start and has
    // no window, ranges are cut into parts at the points (index_parts_plan.h)
    bool fresh = false;
};

namespace {

int index_alloc_windows(flate_hip_ctx* h, flate_hip_index* ix) {
    if (!ix->tab.win_bytes) return FLATE_HIP_OK;
    if (hipMalloc((void**)&ix->d_win, ix->tab.win_bytes) != hipSuccess) {
        (void)hipGetLastError();
        ix->d_win = nullptr;
        h->last_error = "hipMalloc(" + std::to_string(ix->tab.win_bytes) + "): the index's windows";
        return FLATE_HIP_E_ALLOC;
    }
    return FLATE_HIP_OK;
}

// The walk jobs of the good streams of a table (flate_hip_index_build, flate_hip_index_scan): a wave per stream -- a long
// stream a wave per span of the size probe's, where the spans' chain closes; else whole by one wave: always correct, only
// slow.  have: the span records of a size probe that has just run over the same batch (else the spans are counted here).  d_in: the batch on the device, in_shift what its offsets are less than the caller's.  A job has room for the
// points fl_idx_max_points allows its bytes; jobs [job0[i], job0[i + 1]) are stream i's.
int index_walk_jobs(flate_hip_ctx* h, const fl_idx_tab& t, const uint8_t* d_in, const std::vector<uint64_t>& hin, uint64_t in_shift,
                    int container, int flags, std::vector<fl_idx_walk_job>& jobs, std::vector<uint32_t>& job0, uint64_t& cap_total,
                    const SpanRecords* have = nullptr) {
    hipStream_t st = h->stream;
    const uint32_t n = (uint32_t)t.streams.size();
    int rc;
    std::vector<fl_chunk> chunks;  // (the streams' lengths are hin's: the callers took them from it)
    if (!fl_inflate_chunks(hin.data(), nullptr, n, in_shift, 0, chunks)) return FLATE_HIP_E_INVALID_ARG;
    for (uint32_t i = 0; i < n; i++) chunks[i].skip = t.streams[i].status != 0;  // (not walked, and not cut below)
    if ((rc = upload_chunks(h, chunks))) return rc;
    // ---- long streams: the size probe's spans, and where their chain closes a walk per live span
    std::vector<std::vector<fl_idx_span_walk>> cut(n);
    {
        SpanRecords own;
        if (!have) {
            own.nsp = size_span_records(h, st, d_in, chunks, container, flags, own.elig, own.spans, own.sp_first, own.recs);
            if (own.nsp < 0) {
                h->last_error = std::string("index walk by spans: ") + hipGetErrorString(hipGetLastError());
                return FLATE_HIP_E_LAUNCH;
            }
            have = &own;
        }
        // (records of a probe that looked at every stream: those of a stream that failed are passed over)
        for (size_t k = 0; have->nsp > 0 && k < have->elig.size(); k++) {
            const uint32_t a = have->sp_first[k], b = have->sp_first[k + 1], i = have->elig[k];
            if (b - a >= 2 && t.streams[i].status == 0)
                fl_idx_span_walks(have->spans.data() + a, have->recs.data() + a, b - a, t.streams[i].size, t.spacing, cut[i]);
        }
    }
    jobs.clear();
    job0.assign(n + 1, 0);
    cap_total = 0;
    h->dbg_index_spans = h->dbg_index_whole = 0;
    for (uint32_t i = 0; i < n; i++) {
        job0[i] = (uint32_t)jobs.size();
        if (t.streams[i].status != 0) continue;
        if (cut[i].empty()) cut[i].push_back(fl_idx_span_walk{0, ~0ull, 0, fl_idx_max_points(t.streams[i].size, t.spacing), 1});
        (cut[i].size() > 1 ? h->dbg_index_spans : h->dbg_index_whole)++;
        for (const fl_idx_span_walk& w : cut[i]) {
            fl_idx_walk_job jb{};
            jb.start_bit = w.start_bit;
            jb.stop_bit = w.stop_bit;
            jb.base = w.base;
            jb.point0 = cap_total;
            jb.cap = w.cap;
            jb.stream = i;
            jb.first = w.first;
            cap_total += jb.cap;
            jobs.push_back(jb);
        }
    }
    job0[n] = (uint32_t)jobs.size();
    return FLATE_HIP_OK;
}

// The block starts of the streams the build found good, walked by the jobs above, and the windows copied out of the
// decoded bytes.  d_in / d_out:
// the batch on the device, in_shift / out_shift what their offsets are less than the caller's.
int index_walk(flate_hip_ctx* h, flate_hip_index* ix, const uint8_t* d_in, const uint8_t* d_out, const std::vector<uint64_t>& hin,
               const std::vector<uint64_t>& hout, uint64_t in_shift, uint64_t out_shift, int container, int flags) {
    hipStream_t st = h->stream;
    fl_idx_tab& t = ix->tab;
    const uint32_t n = (uint32_t)t.streams.size();
    int rc;
    std::vector<fl_idx_walk_job> jobs;
    std::vector<uint32_t> job0;  // the jobs of stream i: [job0[i], job0[i + 1])
    uint64_t cap_total = 0;
    if ((rc = index_walk_jobs(h, t, d_in, hin, in_shift, container, flags, jobs, job0, cap_total))) return rc;
    const uint32_t nj = (uint32_t)jobs.size();
    if (!nj) return FLATE_HIP_OK;
    if ((rc = ensure(h, h->ix_jobs, sizeof(fl_idx_walk_job) * nj)) || (rc = ensure(h, h->ix_recs, sizeof(fl_idx_walk_rec) * nj)) ||
        (rc = ensure(h, h->ix_ptbit, sizeof(uint64_t) * cap_total)) || (rc = ensure(h, h->ix_ptpos, sizeof(uint64_t) * cap_total)))
        return rc;
    HIP_OK(h, hipMemcpyAsync(h->ix_jobs.p, jobs.data(), sizeof(fl_idx_walk_job) * nj, hipMemcpyHostToDevice, st));
    {
        ProfScope ps(h, K_INDEX_WALK);
        hipLaunchKernelGGL(k_index_walk, dim3(nj), dim3(64), 0, st, d_in, (const fl_chunk*)h->chunks.p, container, flags, t.spacing,
                           (const fl_idx_walk_job*)h->ix_jobs.p, (fl_idx_walk_rec*)h->ix_recs.p, (uint64_t*)h->ix_ptbit.p,
                           (uint64_t*)h->ix_ptpos.p);
    }
    HIP_OK(h, hipGetLastError());
    std::vector<fl_idx_walk_rec> recs(nj);
    std::vector<uint64_t> bit(cap_total), pos(cap_total);
    HIP_OK(h, hipMemcpyAsync(recs.data(), h->ix_recs.p, sizeof(fl_idx_walk_rec) * nj, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(bit.data(), h->ix_ptbit.p, sizeof(uint64_t) * cap_total, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipMemcpyAsync(pos.data(), h->ix_ptpos.p, sizeof(uint64_t) * cap_total, hipMemcpyDeviceToHost, st));
    HIP_OK(h, hipStreamSynchronize(st));
    // ---- the tables, and where every window comes from and goes
    std::vector<uint64_t> wtab;  // src | len | dst, a row each
    for (uint32_t i = 0; i < n; i++) {
        if (job0[i] == job0[i + 1]) continue;
        fl_idx_stream& s = t.streams[i];
        s.point0 = t.points.size();
        uint64_t total = 0;
        bool good = true;
        for (uint32_t k = job0[i]; k < job0[i + 1] && good; k++) {
            const fl_idx_walk_job& jb = jobs[k];
            const fl_idx_walk_rec& r = recs[k];
            good = r.status == 0 && r.n_points <= jb.cap && jb.base == total && (r.final_seen != 0) == (k + 1 == job0[i + 1]);
            total += r.out_len;
            for (uint64_t q = 0; good && q < r.n_points; q++) {
                fl_idx_point p;
                p.in_bit = bit[jb.point0 + q];
                p.out_pos = pos[jb.point0 + q];
                p.win_off = t.win_bytes;
                t.win_bytes += fl_idx_window_len(p.out_pos);
                t.points.push_back(p);
            }
        }
        s.n_points = t.points.size() - s.point0;
        if (!good || total != s.size || s.n_points < 1) {
            h->last_error = "index walk of stream " + std::to_string(i) + " disagrees with its decode";
            return FLATE_HIP_E_LAUNCH;
        }
    }
    const uint64_t np = t.points.size();
    wtab.resize(3 * np);
    for (uint32_t i = 0; i < n; i++) {
        const fl_idx_stream& s = t.streams[i];
        for (uint64_t q = s.point0; q < s.point0 + s.n_points; q++) {
            const fl_idx_point& p = t.points[q];
            const uint64_t wl = fl_idx_window_len(p.out_pos);
            wtab[q] = (hout[i] - out_shift) + p.out_pos - wl;
            wtab[np + q] = wl;
            wtab[2 * np + q] = p.win_off;
        }
    }
    if (!t.win_bytes) return FLATE_HIP_OK;
    if ((rc = index_alloc_windows(h, ix)) || (rc = ensure(h, h->ix_wtab, sizeof(uint64_t) * 3 * np))) return rc;
    HIP_OK(h, hipMemcpyAsync(h->ix_wtab.p, wtab.data(), sizeof(uint64_t) * 3 * np, hipMemcpyHostToDevice, st));
    {
        ProfScope ps(h, K_INDEX_WINDOWS);
        const uint64_t* w = (const uint64_t*)h->ix_wtab.p;
        // (the grid's x is a 32-bit count of workgroups: rounds of points)
        for (uint64_t q0 = 0; q0 < np; q0 += 1u << 20) {
            const uint32_t nq = (uint32_t)std::min<uint64_t>(np - q0, 1u << 20);
            hipLaunchKernelGGL(k_index_windows, dim3(nq, FL_IDX_WINDOW / FL_GATHER_SLICE), dim3(256), 0, st, d_out, w + q0, w + np + q0,
                               ix->d_win, w + 2 * np + q0);
        }
    }
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, hipStreamSynchronize(st));  // (the tables are on this stack; the caller may reuse `out` at once)
    return FLATE_HIP_OK;
}

// flate_hip_index_scan behind its probe (index_scan_plan.h, kernels_index_scan.h): the good streams are walked by the
// jobs of index_walk, cut by the span records the probe has just read back (sr), and every stream's lists become its
// points.  Nothing but the handle's workspace is written.  The lists come home as they are where there is little room
// for them, else only what the walkers wrote, packed on the device behind a look at their records.
int index_scan_walk(flate_hip_ctx* h, flate_hip_index* ix, const uint8_t* d_in, const std::vector<uint64_t>& hin, uint64_t in_shift,
                    int container, int flags, const SpanRecords& sr) {
    hipStream_t st = h->stream;
    fl_idx_tab& t = ix->tab;
    const uint32_t n = (uint32_t)t.streams.size();
    int rc;
    std::vector<fl_idx_walk_job> jobs;
    std::vector<uint32_t> job0;
    uint64_t cap_total = 0;
    if ((rc = index_walk_jobs(h, t, d_in, hin, in_shift, container, flags, jobs, job0, cap_total, &sr))) return rc;
    cap_total = 0;
    for (fl_idx_walk_job& jb : jobs) {  // room for a walk's list, not for its points: by its cells and by its bits
        const uint64_t from = jb.first ? 0 : jb.start_bit, to = jb.stop_bit == ~0ull ? t.streams[jb.stream].in_len * 8 : jb.stop_bit;
        jb.cap = fl_ixs_walk_entries(jb.cap, to - from);
        jb.point0 = cap_total;
        cap_total += jb.cap;
    }
    const uint32_t nj = (uint32_t)jobs.size();
    std::vector<fl_ixs_walk_rec> recs(nj);
    std::vector<fl_ixs_entry> ent;
    std::vector<uint64_t> at(nj, 0);  // where walk k's list begins in `ent`
    if (nj) {
        if ((rc = ensure(h, h->ix_jobs, sizeof(fl_idx_walk_job) * nj)) || (rc = ensure(h, h->ix_recs, sizeof(fl_ixs_walk_rec) * nj)) ||
            (rc = ensure(h, h->ix_entries, sizeof(fl_ixs_entry) * cap_total)))
            return rc;
        HIP_OK(h, hipMemcpyAsync(h->ix_jobs.p, jobs.data(), sizeof(fl_idx_walk_job) * nj, hipMemcpyHostToDevice, st));
        {
            ProfScope ps(h, K_INDEX_SCAN);
            hipLaunchKernelGGL(k_index_scan, dim3(nj), dim3(64), 0, st, d_in, (const fl_chunk*)h->chunks.p, container, flags, t.spacing,
                               (const fl_idx_walk_job*)h->ix_jobs.p, (fl_ixs_walk_rec*)h->ix_recs.p, (fl_ixs_entry*)h->ix_entries.p);
        }
        HIP_OK(h, hipGetLastError());
        HIP_OK(h, hipMemcpyAsync(recs.data(), h->ix_recs.p, sizeof(fl_ixs_walk_rec) * nj, hipMemcpyDeviceToHost, st));
        const bool whole = cap_total <= FL_IXS_COPY_WHOLE;
        if (whole) {
            ent.resize(cap_total);
            HIP_OK(h, hipMemcpyAsync(ent.data(), h->ix_entries.p, sizeof(fl_ixs_entry) * cap_total, hipMemcpyDeviceToHost, st));
            for (uint32_t k = 0; k < nj; k++) at[k] = jobs[k].point0;
        }
        HIP_OK(h, hipStreamSynchronize(st));
        if (!whole) {
            std::vector<uint64_t> tab(3 * (size_t)nj);  // k_gather_copy's: source | length | destination, in bytes
            uint64_t total = 0;
            for (uint32_t k = 0; k < nj; k++) {
                at[k] = total;
                tab[k] = sizeof(fl_ixs_entry) * jobs[k].point0;
                tab[nj + k] = sizeof(fl_ixs_entry) * std::min(recs[k].n_entries, jobs[k].cap);
                tab[2 * (size_t)nj + k] = sizeof(fl_ixs_entry) * total;
                total += std::min(recs[k].n_entries, jobs[k].cap);
            }
            ent.resize(total);
            if (total) {
                if ((rc = ensure(h, h->ix_wtab, sizeof(uint64_t) * 3 * nj)) || (rc = ensure(h, h->ix_epack, sizeof(fl_ixs_entry) * total))) return rc;
                HIP_OK(h, hipMemcpyAsync(h->ix_wtab.p, tab.data(), sizeof(uint64_t) * 3 * nj, hipMemcpyHostToDevice, st));
                const uint64_t* w = (const uint64_t*)h->ix_wtab.p;
                {
                    ProfScope ps(h, K_GATHER);
                    hipLaunchKernelGGL(k_gather_copy, gather_grid(nj), dim3(256), 0, st, (const uint8_t*)h->ix_entries.p, w, w + nj,
                                       (uint8_t*)h->ix_epack.p, w + 2 * (size_t)nj);
                }
                HIP_OK(h, hipGetLastError());
                HIP_OK(h, hipMemcpyAsync(ent.data(), h->ix_epack.p, sizeof(fl_ixs_entry) * total, hipMemcpyDeviceToHost, st));
                HIP_OK(h, hipStreamSynchronize(st));  // (the table is on this stack)
            }
        }
    }
    std::vector<fl_ixs_walk> walks;
    for (uint32_t i = 0; i < n; i++) {
        fl_idx_stream& s = t.streams[i];
        s.point0 = t.points.size();
        s.n_points = 0;
        if (job0[i] == job0[i + 1]) continue;
        walks.clear();
        bool good = true;
        for (uint32_t k = job0[i]; k < job0[i + 1] && good; k++) {
            const fl_idx_walk_job& jb = jobs[k];
            const fl_ixs_walk_rec& r = recs[k];
            good = r.status == 0 && r.n_entries <= jb.cap && (r.final_seen != 0) == (k + 1 == job0[i + 1]);
            walks.push_back(fl_ixs_walk{ent.data() + at[k], r.n_entries, r.out_len, r.last_mark, r.has_mark, jb.first});
        }
        if (!good || !fl_ixs_points(walks.data(), walks.size(), s.size, t.spacing, t.points)) {
            h->last_error = "index scan of stream " + std::to_string(i) + " disagrees with its probe";
            return FLATE_HIP_E_LAUNCH;
        }
        s.n_points = t.points.size() - s.point0;
    }
    return FLATE_HIP_OK;
}

// flate_hip_decompress_ranges on a fresh index (index_parts_plan.h: the cut, the part table, the passes).  The offsets and
// the range arrays are on the host already.  The host waits behind the upload of the tables; the parts of a pass are
// decoded a wave each (k_inflate_part), its scratch parts copied to their slots (k_range_pack), and behind the last pass
// k_range_settle gives every range its status and length; a host caller's results come home packed, slot by slot.
int ranges_by_parts(flate_hip_ctx* h, const fl_idx_tab& t, const uint8_t* in, const std::vector<uint64_t>& hin, uint32_t n_ranges,
                    const std::vector<uint32_t>& hstream, const std::vector<uint64_t>& hbegin, const std::vector<uint64_t>& hlen,
                    uint8_t* out, const std::vector<uint64_t>& hout, uint64_t* out_len, int32_t* status, int memkind) {
    hipStream_t st = h->stream;
    int rc;
    fl_idxp_call c;
    if (!fl_idxp_plan_call(t, n_ranges, hstream.data(), hbegin.data(), hlen.data(), hout.data(), h->knobs.index_pass_bytes, c))
        return FLATE_HIP_E_UNSUPPORTED;
    const size_t np = c.parts.size();
    h->dbg_index_direct = c.n_direct;
    h->dbg_index_scratch = c.n_scratch;

    InflateFrame f(h, memkind, n_ranges);
    f.input(in, hin[0], hin[hin.size() - 1]).output(out, hout[0], hout[n_ranges]).results(out_len, status, nullptr);
    if (f.host) {
        // of the input only what the parts can consume is staged, each byte at its own place: from a part's point to the
        // next point
        std::vector<uint64_t> iv;
        for (const fl_idxp_part& p : c.parts) {
            iv.push_back(hin[hstream[p.range]] + p.in_lo);
            iv.push_back(hin[hstream[p.range]] + p.in_hi);
        }
        fl_idx_merge_intervals(iv, 65536);
        if ((rc = reserve_frame(f, FRAME_OUT)) || (rc = stage_frame(f, FRAME_OUT, iv.data(), iv.size()))) return rc;
    }
    std::vector<fl_part_job> jobs(np);
    std::vector<uint64_t> ptab(2 * np);  // the pack kernel's: source in the scratch | destination
    std::vector<fl_range_rec> recs(n_ranges);
    std::vector<uint64_t> rdst(n_ranges);
    for (size_t k = 0; k < np; k++) {
        const fl_idxp_part& p = c.parts[k];
        const fl_idx_point& pt = t.points[p.point];
        const uint32_t si = hstream[p.range];
        const uint64_t dst = (hout[p.range] - f.out_shift) + p.dst;
        fl_part_job jb{};
        jb.in_off = hin[si] - f.in_shift;
        jb.in_len = (uint32_t)t.streams[si].in_len;
        jb.in_bit = pt.in_bit;
        jb.dst_off = p.direct ? dst : c.slot_off[k];
        jb.need = p.skip + p.len;
        jb.len = p.len;
        jb.direct = p.direct;
        jobs[k] = jb;
        ptab[k] = c.slot_off[k] + p.skip;
        ptab[np + k] = dst;
    }
    for (uint32_t j = 0; j < n_ranges; j++) {
        recs[j] = fl_range_rec{c.ranges[j].part0, c.ranges[j].n_parts, c.ranges[j].len, c.ranges[j].status, 0};
        rdst[j] = hout[j] - f.out_shift;
    }
    if ((rc = ensure(h, h->ix_pjobs, sizeof(fl_part_job) * np + 16)) || (rc = ensure(h, h->ix_ptab, sizeof(uint64_t) * 2 * np + 16)) ||
        (rc = ensure(h, h->ix_plen, sizeof(uint64_t) * np + 16)) || (rc = ensure(h, h->ix_pstatus, sizeof(int32_t) * np + 16)) ||
        (rc = ensure(h, h->ix_rrec, sizeof(fl_range_rec) * n_ranges)) || (rc = ensure(h, h->ix_rdst, sizeof(uint64_t) * n_ranges)) ||
        (rc = ensure(h, h->ix_scratch, c.scratch + 16)))
        return rc;
    if (np) {
        HIP_OK(h, hipMemcpyAsync(h->ix_pjobs.p, jobs.data(), sizeof(fl_part_job) * np, hipMemcpyHostToDevice, st));
        HIP_OK(h, hipMemcpyAsync(h->ix_ptab.p, ptab.data(), sizeof(uint64_t) * 2 * np, hipMemcpyHostToDevice, st));
    }
    HIP_OK(h, hipMemcpyAsync(h->ix_rrec.p, recs.data(), sizeof(fl_range_rec) * n_ranges, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->ix_rdst.p, rdst.data(), sizeof(uint64_t) * n_ranges, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));  // (the tables are on the host's stack)

    // ---- the passes, one after the other in the stream: they share the scratch
    const fl_part_job* dj = (const fl_part_job*)h->ix_pjobs.p;
    const uint64_t* dsrc = (const uint64_t*)h->ix_ptab.p;
    const uint64_t* ddst = dsrc + np;
    uint64_t* dlen = (uint64_t*)h->ix_plen.p;
    int32_t* dstat = (int32_t*)h->ix_pstatus.p;
    uint8_t* dscr = (uint8_t*)h->ix_scratch.p;
    for (size_t k = 0; k + 1 < c.pass_first.size(); k++) {
        const size_t a = (size_t)c.pass_first[k];
        const uint32_t n = (uint32_t)(c.pass_first[k + 1] - c.pass_first[k]);
        uint64_t longest = 0;  // among the pass's scratch parts
        for (size_t q = a; q < a + n; q++)
            if (!c.parts[q].direct) longest = std::max(longest, c.parts[q].len);
        {
            ProfScope ps(h, K_INFLATE_PART);
            const auto kern = fl_inflate_ring_large(h->knobs.inflate_ring, n) ? k_inflate_part<FL_INF_RING_LARGE> : k_inflate_part<FL_INF_RING_SMALL>;
            hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, st, f.d_in, dj + a, 0, dscr, f.d_out, dlen + a, dstat + a);
        }
        if (longest) {
            ProfScope ps(h, K_RANGE_PACK);
            const uint32_t ny = (uint32_t)std::min<uint64_t>(16, (longest + FL_GATHER_SLICE - 1) / FL_GATHER_SLICE);
            hipLaunchKernelGGL(k_range_pack, dim3(n, ny), dim3(256), 0, st, (const uint8_t*)dscr, dsrc + a, (const uint64_t*)(dlen + a), f.d_out,
                               ddst + a);
        }
        HIP_OK(h, hipGetLastError());
        h->dbg_index_passes++;
    }
    {
        ProfScope ps(h, K_RANGE_SETTLE);
        hipLaunchKernelGGL(k_range_settle, dim3(n_ranges), dim3(64), 0, st, (const fl_range_rec*)h->ix_rrec.p, (const int32_t*)dstat, f.d_outlen,
                           f.d_status);
    }
    HIP_OK(h, hipGetLastError());
    if ((rc = results_home(f, out_len, status, nullptr)) || (rc = wait_for_results(f)) || !f.host) return rc;
    // the delivered bytes back to back, then slot by slot: nothing else of the caller's buffer is written
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_ranges; j++) total += out_len[j];
    return total ? copy_out_packed(h, f.d_out, (const uint64_t*)h->ix_rdst.p, f.d_outlen, n_ranges, hout, f.out_shift, out, out_len, total)
                 : FLATE_HIP_OK;
}

}  // namespace

extern "C" {

// flate_hip_compress_joined, with the places of the point pieces read back (index_parts_plan.h: which pieces, what the
// points are).  The host waits for the stream, then, device memory, for out_len and status.
int flate_hip_compress_joined_indexed(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                                      uint32_t piece_bytes, int container, int mode, uint8_t* out, const uint64_t* out_off,
                                      uint64_t* out_len, int32_t* status, int memkind, uint64_t spacing, flate_hip_index_t* idx) {
    if (!idx) return FLATE_HIP_E_INVALID_ARG;
    *idx = nullptr;
    JoinIndex ji;
    ji.spacing = spacing;
    int rc = joined_impl(h, in, in_off, n_streams, piece_bytes, container, mode, out, out_off, out_len, status, memkind, &ji);
    if (rc) return rc;
    std::vector<uint64_t> hlen;
    std::vector<int32_t> hst;
    if (n_streams && ((rc = fetch_array(h, out_len, n_streams, memkind, hlen)) || (rc = fetch_array(h, status, n_streams, memkind, hst))))
        return rc;
    for (uint32_t i = 0; i < n_streams; i++)
        if (hlen[i] > FL_IDX_MAX_IN_LEN) {  // (no decompress call takes such a stream)
            h->last_error = "joined stream " + std::to_string(i) + " is too long for a seek index";
            return FLATE_HIP_E_UNSUPPORTED;
        }
    const uint32_t piece = fl_join_piece_bytes(piece_bytes);
    flate_hip_index* ix = new flate_hip_index();
    ix->fresh = true;
    ix->tab.container = (uint32_t)container;
    ix->tab.spacing = fl_idx_spacing(spacing);
    ix->tab.streams.resize(n_streams);
    uint64_t q0 = 0;
    for (uint32_t i = 0; i < n_streams; i++) {
        fl_idx_stream& s = ix->tab.streams[i];
        const uint64_t nq = ji.n_which[i];
        s.in_len = hlen[i];
        s.status = hst[i];
        s.size = 0;
        s.point0 = ix->tab.points.size();
        s.n_points = 0;
        if (hst[i] == 0) {  // (a failed stream has no points: a piece of it may not inflate to `piece` bytes)
            s.size = ji.streams[i].n;
            for (uint64_t q = q0; q < q0 + nq; q++) ji.place[q] -= ji.streams[i].out_off;
            fl_idxp_points(ji.which.data() + q0, ji.place.data() + q0, nq, piece, ix->tab.points);
            s.n_points = nq;
        }
        q0 += nq;
    }
    *idx = ix;
    return FLATE_HIP_OK;
}

// flate_hip_decompress_batch, then the walk over what it decoded.  The host waits as that call does, then for out_len and
// status (device memory), for the walkers' records and points, and for the window copies.
int flate_hip_index_build(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams, int container, int flags,
                          uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, uint64_t* consumed, int memkind,
                          uint64_t spacing, flate_hip_index_t* idx) {
    if (!idx) return FLATE_HIP_E_INVALID_ARG;
    *idx = nullptr;
    if (!h || !in_off || !out_off || !out_len || !status) return FLATE_HIP_E_INVALID_ARG;
    if (!fl_idx_args_ok(container, memkind)) return FLATE_HIP_E_INVALID_ARG;
    int rc;
    std::vector<uint64_t> hin(1, 0), hout(1, 0), hlen;
    std::vector<int32_t> hst;
    if (n_streams) {
        if ((rc = flate_hip_decompress_batch(h, in, in_off, n_streams, container, flags, out, out_off, out_len, status, consumed, memkind)))
            return rc;
        if ((rc = fetch_offsets(h, in_off, n_streams, memkind, hin)) || (rc = fetch_offsets(h, out_off, n_streams, memkind, hout)) ||
            (rc = fetch_array(h, out_len, n_streams, memkind, hlen)) || (rc = fetch_array(h, status, n_streams, memkind, hst)))
            return rc;
    }
    flate_hip_index* ix = new flate_hip_index();
    ix->tab.container = (uint32_t)container;
    ix->tab.spacing = fl_idx_spacing(spacing);
    ix->tab.streams.resize(n_streams);
    for (uint32_t i = 0; i < n_streams; i++) {
        fl_idx_stream& s = ix->tab.streams[i];
        s.in_len = hin[i + 1] - hin[i];
        s.status = hst[i];
        s.size = hst[i] == 0 ? hlen[i] : 0;
        s.point0 = s.n_points = 0;
    }
    if (n_streams) {
        // a host caller's batch is still where flate_hip_decompress_batch staged and decoded it
        const bool host = memkind == FLATE_HIP_MEM_HOST;
        rc = index_walk(h, ix, host ? (const uint8_t*)h->st_in.p : in, host ? (const uint8_t*)h->st_out.p : out, hin, hout,
                        host ? hin[0] : 0, host ? hout[0] : 0, container, flags);
        if (rc) {
            if (ix->d_win) (void)hipFree(ix->d_win);
            delete ix;
            return rc;
        }
    }
    *idx = ix;
    return FLATE_HIP_OK;
}

// flate_hip_decompressed_sizes, then the scan walk over the streams it found good.  The host waits as that call does, then
// for the offsets, sizes and status (device memory), for the walkers' records, and for their lists.
int flate_hip_index_scan(flate_hip_handle h, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams, int container, int flags,
                         uint64_t* sizes, int32_t* status, uint64_t* consumed, int memkind, uint64_t spacing, flate_hip_index_t* idx) {
    if (!idx) return FLATE_HIP_E_INVALID_ARG;
    *idx = nullptr;
    if (!h || !in_off || !sizes || !status) return FLATE_HIP_E_INVALID_ARG;
    if (!fl_idx_args_ok(container, memkind)) return FLATE_HIP_E_INVALID_ARG;
    int rc;
    std::vector<uint64_t> hin(1, 0), hsize;
    std::vector<int32_t> hst;
    SpanRecords sr;
    if (n_streams) {
        if ((rc = sizes_impl(h, in, in_off, n_streams, container, flags, sizes, status, consumed, memkind, &sr))) return rc;
        if ((rc = fetch_offsets(h, in_off, n_streams, memkind, hin)) || (rc = fetch_array(h, sizes, n_streams, memkind, hsize)) ||
            (rc = fetch_array(h, status, n_streams, memkind, hst)))
            return rc;
        for (uint32_t i = 0; i < n_streams; i++)
            if (hin[i + 1] - hin[i] > FL_IDX_MAX_IN_LEN) {  // (no decompress call takes such a stream)
                h->last_error = "stream " + std::to_string(i) + " is too long for a seek index";
                return FLATE_HIP_E_UNSUPPORTED;
            }
    }
    flate_hip_index* ix = new flate_hip_index();
    ix->fresh = true;
    ix->tab.container = (uint32_t)container;
    ix->tab.spacing = fl_idx_spacing(spacing);
    ix->tab.streams.resize(n_streams);
    for (uint32_t i = 0; i < n_streams; i++) {
        fl_idx_stream& s = ix->tab.streams[i];
        s.in_len = hin[i + 1] - hin[i];
        s.status = hst[i];
        s.size = hst[i] == 0 ? hsize[i] : 0;
        s.point0 = s.n_points = 0;
    }
    if (n_streams) {
        // a host caller's batch is still where flate_hip_decompressed_sizes staged it
        const bool host = memkind == FLATE_HIP_MEM_HOST;
        rc = index_scan_walk(h, ix, host ? (const uint8_t*)h->st_in.p : in, hin, host ? hin[0] : 0, container, flags, sr);
        if (rc) {
            delete ix;
            return rc;
        }
    }
    *idx = ix;
    return FLATE_HIP_OK;
}

int flate_hip_index_destroy(flate_hip_handle h, flate_hip_index_t idx) {
    if (!h || !idx) return FLATE_HIP_E_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (idx->d_win) (void)hipFree(idx->d_win);
    delete idx;
    return FLATE_HIP_OK;
}

int flate_hip_index_stream_info(flate_hip_handle h, flate_hip_index_t idx, uint32_t stream, uint64_t* size, int32_t* status,
                                uint64_t* n_points) {
    if (!h || !idx || stream >= idx->tab.streams.size()) return FLATE_HIP_E_INVALID_ARG;
    const fl_idx_stream& s = idx->tab.streams[stream];
    if (size) *size = s.size;
    if (status) *status = s.status;
    if (n_points) *n_points = s.n_points;
    return FLATE_HIP_OK;
}

int64_t flate_hip_index_points(flate_hip_handle h, flate_hip_index_t idx, uint32_t stream, uint64_t* in_bit, uint64_t* out_pos,
                               uint64_t cap) {
    if (!h || !idx || stream >= idx->tab.streams.size()) return FLATE_HIP_E_INVALID_ARG;
    const fl_idx_stream& s = idx->tab.streams[stream];
    for (uint64_t k = 0; k < s.n_points && k < cap; k++) {
        if (in_bit) in_bit[k] = idx->tab.points[s.point0 + k].in_bit;
        if (out_pos) out_pos[k] = idx->tab.points[s.point0 + k].out_pos;
    }
    return (int64_t)s.n_points;
}

int flate_hip_index_export_size(flate_hip_handle h, flate_hip_index_t idx, uint64_t* bytes) {
    if (!h || !idx || !bytes) return FLATE_HIP_E_INVALID_ARG;
    *bytes = idx->fresh ? fl_idxp_blob_bytes(idx->tab) : fl_idx_blob_bytes(idx->tab);
    return FLATE_HIP_OK;
}

int flate_hip_index_export(flate_hip_handle h, flate_hip_index_t idx, uint8_t* blob_host, uint64_t cap) {
    if (!h || !idx || !blob_host) return FLATE_HIP_E_INVALID_ARG;
    if (idx->fresh) {  // (tables alone: nothing of it is on the device)
        if (cap < fl_idxp_blob_bytes(idx->tab)) return FLATE_HIP_E_INVALID_ARG;
        (void)fl_idxp_blob_write(idx->tab, blob_host);
        return FLATE_HIP_OK;
    }
    if (cap < fl_idx_blob_bytes(idx->tab)) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    const uint64_t at = fl_idx_blob_write(idx->tab, blob_host);
    if (idx->tab.win_bytes) {
        HIP_OK(h, hipMemcpyAsync(blob_host + at, idx->d_win, idx->tab.win_bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_OK(h, hipStreamSynchronize(h->stream));
    }
    return FLATE_HIP_OK;
}

int flate_hip_index_import(flate_hip_handle h, const uint8_t* blob_host, uint64_t bytes, flate_hip_index_t* idx) {
    if (!idx) return FLATE_HIP_E_INVALID_ARG;
    *idx = nullptr;
    if (!h || !blob_host) return FLATE_HIP_E_INVALID_ARG;
    flate_hip_index* ix = new flate_hip_index();
    uint64_t at = 0;
    // (the version field picks the parser; each refuses every version but its own)
    ix->fresh = fl_idxp_blob_version(blob_host, bytes) == FL_IDXP_VERSION;
    if (!(ix->fresh ? fl_idxp_blob_parse(blob_host, bytes, ix->tab) : fl_idx_blob_parse(blob_host, bytes, ix->tab, &at))) {
        delete ix;
        return FLATE_HIP_E_INVALID_ARG;
    }
    int rc = hipSetDevice(h->device) != hipSuccess ? FLATE_HIP_E_NO_DEVICE : index_alloc_windows(h, ix);
    if (!rc && ix->tab.win_bytes) {
        if (hipMemcpyAsync(ix->d_win, blob_host + at, ix->tab.win_bytes, hipMemcpyHostToDevice, h->stream) != hipSuccess ||
            hipStreamSynchronize(h->stream) != hipSuccess) {
            h->last_error = std::string("index import: ") + hipGetErrorString(hipGetLastError());
            rc = FLATE_HIP_E_LAUNCH;
        }
    }
    if (rc) {
        if (ix->d_win) (void)hipFree(ix->d_win);
        delete ix;
        return rc;
    }
    *idx = ix;
    return FLATE_HIP_OK;
}

// The host waits for the offsets and the three range arrays (device memory), plans every range (index_plan.h), and waits
// once more behind the upload of the job tables; a host caller's results come home packed, slot by slot.
int flate_hip_decompress_ranges(flate_hip_handle h, flate_hip_index_t idx, const uint8_t* in, const uint64_t* in_off, uint32_t n_streams,
                                uint32_t n_ranges, const uint32_t* range_stream, const uint64_t* range_begin, const uint64_t* range_len,
                                uint8_t* out, const uint64_t* out_off, uint64_t* out_len, int32_t* status, int memkind) {
    if (!h || !idx || !in_off) return FLATE_HIP_E_INVALID_ARG;
    if (memkind != FLATE_HIP_MEM_HOST && memkind != FLATE_HIP_MEM_DEVICE) return FLATE_HIP_E_INVALID_ARG;
    const fl_idx_tab& t = idx->tab;
    if (n_streams != t.streams.size()) return FLATE_HIP_E_INVALID_ARG;
    if (n_ranges && (!range_stream || !range_begin || !range_len || !out_off || !out_len || !status)) return FLATE_HIP_E_INVALID_ARG;
    if (hipSetDevice(h->device) != hipSuccess) return FLATE_HIP_E_NO_DEVICE;
    hipStream_t st = h->stream;
    int rc;
    std::vector<uint64_t> hin(1, 0), hout, hbegin, hlen;
    std::vector<uint32_t> hstream;
    if (n_streams && (rc = fetch_offsets(h, in_off, n_streams, memkind, hin))) return rc;
    for (uint32_t i = 0; i < n_streams; i++)
        if (hin[i + 1] - hin[i] != t.streams[i].in_len) return FLATE_HIP_E_INVALID_ARG;
    h->dbg_index_passes = h->dbg_index_direct = h->dbg_index_scratch = 0;
    if (n_ranges == 0) return FLATE_HIP_OK;
    if ((rc = fetch_offsets(h, out_off, n_ranges, memkind, hout)) || (rc = fetch_array(h, range_stream, n_ranges, memkind, hstream)) ||
        (rc = fetch_array(h, range_begin, n_ranges, memkind, hbegin)) || (rc = fetch_array(h, range_len, n_ranges, memkind, hlen)))
        return rc;
    for (uint32_t j = 0; j < n_ranges; j++)
        if (hstream[j] >= n_streams) return FLATE_HIP_E_INVALID_ARG;
    const uint64_t in_lo = hin[0], in_hi = hin[n_streams], out_lo = hout[0], out_hi = hout[n_ranges];
    if ((in_hi > in_lo && !in) || (out_hi > out_lo && !out)) return FLATE_HIP_E_INVALID_ARG;
    if (idx->fresh) return ranges_by_parts(h, t, in, hin, n_ranges, hstream, hbegin, hlen, out, hout, out_len, status, memkind);

    // ---- every range: its point, what it skips and delivers, its scratch; the passes
    std::vector<fl_idx_range> plan(n_ranges);
    std::vector<uint64_t> slot(n_ranges), pass_first, slot_off;
    for (uint32_t j = 0; j < n_ranges; j++) {
        plan[j] = fl_idx_plan_range(t, hstream[j], hbegin[j], hlen[j], hout[j + 1] - hout[j]);
        slot[j] = plan[j].decode ? fl_idx_slot_bytes(plan[j].skip + plan[j].len) : 0;
    }
    const uint64_t scratch = fl_idx_passes(slot.data(), n_ranges, h->knobs.index_pass_bytes, pass_first, slot_off);

    InflateFrame f(h, memkind, n_ranges);
    f.input(in, in_lo, in_hi).output(out, out_lo, out_hi).results(out_len, status, nullptr);
    if (f.host) {
        // Of the input only what the decodes can consume is staged, each byte at its own place: from a range's point to
        // the first point at or behind its end.  (The bit reader stages and looks ahead beyond that; what it finds there
        // is never consumed.)
        std::vector<uint64_t> iv;
        for (uint32_t j = 0; j < n_ranges; j++)
            if (plan[j].decode) {
                iv.push_back(hin[hstream[j]] + plan[j].in_lo);
                iv.push_back(hin[hstream[j]] + plan[j].in_hi);
            }
        fl_idx_merge_intervals(iv, 65536);
        if ((rc = reserve_frame(f, FRAME_OUT)) || (rc = stage_frame(f, FRAME_OUT, iv.data(), iv.size()))) return rc;
    }
    std::vector<fl_range_job> jobs(n_ranges);
    std::vector<uint64_t> rtab(2 * (size_t)n_ranges);  // the pack kernel's: source in the scratch | destination
    for (uint32_t j = 0; j < n_ranges; j++) {
        const fl_idx_range& p = plan[j];
        fl_range_job jb{};
        jb.status = p.status;
        jb.decode = p.decode;
        if (p.decode) {
            const fl_idx_point& pt = t.points[p.point];
            jb.in_off = hin[hstream[j]] - f.in_shift;
            jb.in_len = (uint32_t)t.streams[hstream[j]].in_len;
            jb.in_bit = pt.in_bit;
            jb.win_off = pt.win_off;
            jb.win_len = fl_idx_window_len(pt.out_pos);
            jb.slot_off = slot_off[j];
            jb.need = p.skip + p.len;
            jb.len = p.len;
        }
        jobs[j] = jb;
        rtab[j] = slot_off[j] + p.skip;
        rtab[n_ranges + j] = hout[j] - f.out_shift;
    }
    if ((rc = ensure(h, h->ix_rjobs, sizeof(fl_range_job) * n_ranges)) || (rc = ensure(h, h->ix_rtab, sizeof(uint64_t) * 2 * n_ranges)) ||
        (rc = ensure(h, h->ix_scratch, scratch + 16)))
        return rc;
    HIP_OK(h, hipMemcpyAsync(h->ix_rjobs.p, jobs.data(), sizeof(fl_range_job) * n_ranges, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipMemcpyAsync(h->ix_rtab.p, rtab.data(), sizeof(uint64_t) * 2 * n_ranges, hipMemcpyHostToDevice, st));
    HIP_OK(h, hipStreamSynchronize(st));  // (the tables are on the host's stack)

    // ---- the passes, one after the other in the stream: they share the scratch
    const fl_range_job* dj = (const fl_range_job*)h->ix_rjobs.p;
    const uint64_t* dsrc = (const uint64_t*)h->ix_rtab.p;
    const uint64_t* ddst = dsrc + n_ranges;
    uint8_t* dscr = (uint8_t*)h->ix_scratch.p;
    for (size_t k = 0; k + 1 < pass_first.size(); k++) {
        const uint32_t a = (uint32_t)pass_first[k], nr = (uint32_t)(pass_first[k + 1] - pass_first[k]);
        uint64_t longest = 0;
        for (uint32_t j = a; j < a + nr; j++) longest = std::max(longest, plan[j].len);
        {
            ProfScope ps(h, K_INFLATE_RANGE);
            const auto kern = fl_inflate_ring_large(h->knobs.inflate_ring, nr) ? k_inflate_range<FL_INF_RING_LARGE> : k_inflate_range<FL_INF_RING_SMALL>;
            hipLaunchKernelGGL(kern, dim3(nr), dim3(64), 0, st, f.d_in, dj + a, 0, (const uint8_t*)idx->d_win, dscr, f.d_outlen + a,
                               f.d_status + a);
        }
        if (longest) {
            ProfScope ps(h, K_RANGE_PACK);
            const uint32_t ny = (uint32_t)std::min<uint64_t>(16, (longest + FL_GATHER_SLICE - 1) / FL_GATHER_SLICE);
            hipLaunchKernelGGL(k_range_pack, dim3(nr, ny), dim3(256), 0, st, (const uint8_t*)dscr, dsrc + a, (const uint64_t*)(f.d_outlen + a),
                               f.d_out, ddst + a);
        }
        HIP_OK(h, hipGetLastError());
        h->dbg_index_passes++;
    }
    if ((rc = results_home(f, out_len, status, nullptr)) || (rc = wait_for_results(f)) || !f.host) return rc;
    // the delivered bytes back to back, then slot by slot: nothing else of the caller's buffer is written
    uint64_t total = 0;
    for (uint32_t j = 0; j < n_ranges; j++) total += out_len[j];
    return total ? copy_out_packed(h, f.d_out, ddst, f.d_outlen, n_ranges, hout, f.out_shift, out, out_len, total) : FLATE_HIP_OK;
}

// Debug / test seam: the good streams of the last flate_hip_index_build or flate_hip_index_scan call that were walked span by span / whole by one wave.
int flate_hip_debug_index_paths(flate_hip_handle h, uint64_t counts[2]) {
    if (!h || !counts) return FLATE_HIP_E_INVALID_ARG;
    counts[0] = h->dbg_index_spans;
    counts[1] = h->dbg_index_whole;
    return FLATE_HIP_OK;
}

// Debug / test seam: the parts of the last flate_hip_decompress_ranges call (a fresh index; else 0 | 0) that were decoded
// straight into a caller's slot | through scratch.
int flate_hip_debug_index_parts(flate_hip_handle h, uint64_t counts[2]) {
    if (!h || !counts) return FLATE_HIP_E_INVALID_ARG;
    counts[0] = h->dbg_index_direct;
    counts[1] = h->dbg_index_scratch;
    return FLATE_HIP_OK;
}

// Debug / test seam: the passes the last flate_hip_decompress_ranges call took.
int flate_hip_debug_index_passes(flate_hip_handle h, uint64_t* passes) {
    if (!h || !passes) return FLATE_HIP_E_INVALID_ARG;
    *passes = h->dbg_index_passes;
    return FLATE_HIP_OK;
}

}  // extern "C"
