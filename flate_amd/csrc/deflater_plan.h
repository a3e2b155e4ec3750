// deflater_plan.h -- host side of a resumable huffman-only / store-only feed (flate_hip_deflater_*): which blocks
// a stream's buffered bytes plus its new piece turn into and what stays buffered, and every decision a feed takes on
// the host -- the check of the caller's tables, which streams drain pending output, are finished, are skipped or take
// their piece (fl_dfl_route_stream), the jobs, tables and staging layout of those that do (fl_dfl_lay_out), and what
// becomes of the bytes a job produced (fl_dfl_settle).  flate_hip_deflater_feed carries these out.  Plain C++ (no HIP):
// flate_hip.hip and kernels_deflater.h use it, tests/cpu_shim and tests/host_cpp compile it for the CPU tests.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "flate_layout.h"

// device bytes per stream that hold the SimpleCompressor's buffer between feeds (it never holds 65535)
#define FL_DFL_BUF 65536u

// the largest piece one feed takes for a stream: its buffer and the piece are staged together, positions are 32-bit
#define FL_DFL_MAX_PIECE (0xfff00000ull - FL_DFL_BUF)

enum { FL_FEED_MORE = 0, FL_FEED_FLUSH = 1, FL_FEED_FINISH = 2 };

// the statuses of include/flate_hip.h a feed reports (flate_hip.hip asserts that they are)
enum { FL_DFL_ST_OK = 0, FL_DFL_ST_NEED_INPUT = 104, FL_DFL_ST_NEED_OUTPUT = 105 };

// The SimpleCompressor (deflate.zig:449-529) writes its 65535-byte buffer out as a block each time it is full;
// flush() writes what it holds (an empty block if nothing) and an empty stored block, finish() writes it as the final
// block.  `bl` buffered bytes followed by `n` new ones: appends the blocks (staged-input-relative byte ranges,
// fl_sblock flags) to `out` and returns how many bytes at the end stay buffered.  Fed the whole stream at once this is
// the block list of flate_hip_compress_batch (in_len / 65535 + 1 blocks) and, with flushes, of
// flate_hip_compress_flush; cut anywhere, the concatenated lists cover the same bytes with the same blocks.
inline uint32_t fl_dfl_blocks(uint32_t bl, uint32_t n, int op, std::vector<fl_sblock>& out) {
    const uint32_t L = bl + n;
    uint32_t p = 0;
    for (; L - p >= FL_BLOCK_BYTES; p += FL_BLOCK_BYTES) out.push_back(fl_sblock{p, FL_BLOCK_BYTES, 0u});
    if (op == FL_FEED_MORE) return L - p;
    out.push_back(fl_sblock{p, L - p, op == FL_FEED_FINISH ? 1u : 0u});
    if (op == FL_FEED_FLUSH) out.push_back(fl_sblock{0u, 0u, 2u});
    return 0;
}

// The piece's checksum units (k_checksum folds at most 65535 bytes per unit): [bl, bl + n) cut at 65535 bytes
inline uint32_t fl_dfl_checksum_units(uint32_t bl, uint32_t n, std::vector<fl_sblock>& out) {
    uint32_t k = 0;
    for (uint32_t p = 0; p < n; p += FL_BLOCK_BYTES, k++) {
        const uint32_t len = n - p < FL_BLOCK_BYTES ? n - p : FL_BLOCK_BYTES;
        out.push_back(fl_sblock{bl + p, len, 0u});
    }
    return k;
}

// Output bytes a feed of `bl + n` bytes can produce at most: the blocks (stored-block bound: 5 bytes per 65535 and
// two more blocks), the container header and footer, the carried byte.
inline uint64_t fl_dfl_out_bound(uint32_t bl, uint32_t n) {
    const uint64_t L = (uint64_t)bl + n;
    return L + 5 * (L / FL_BLOCK_BYTES + 3) + 10 + 8 + 1 + 16;
}

// ---- one feed

// per stream, host memory: what the feeds plan with, kept beside the device's fl_dfl_state
struct fl_dfl_mirror {
    uint32_t bl = 0;       // bytes in the stream's buffer (< 65535)
    uint8_t hdr_done = 0;  // the container header has gone out
    uint8_t finished = 0;  // a FINISH feed was taken: nothing more until reset
    // output a feed made beyond its slot, handed out by the next feeds before the stream takes more input:
    // pend_len bytes are kept, those before pend_pos have been handed out
    uint64_t pend_len = 0, pend_pos = 0;
};

// per stream fed in this call (host-built, read by the kernels of kernels_deflater.h)
struct fl_dfl_job {
    uint64_t src_off;   // the piece in the feed's source buffer
    uint32_t stream;    // index of the stream in the deflater
    uint32_t bl;        // buffered bytes carried from the last feed (< 65535), staged before the piece
    uint32_t n;         // bytes of the piece
    uint32_t keep;      // bytes at the end of the staged input that stay buffered
    uint32_t ck_first;  // the piece's checksum units in the checksum tables ...
    uint32_t ck_n;      // ... and how many
    uint32_t hdr;       // 1: the container header goes out first
    uint32_t finish;    // 1: final block and footer
};

// The caller's tables, n + 1 offsets each and n ops, on the host: the offsets ascend, no op is above FINISH, no piece is
// longer than FL_DFL_MAX_PIECE, and there is an input buffer where there are input bytes.
inline bool fl_dfl_feed_ok(const uint64_t* hin, const uint64_t* hout, const uint8_t* hop, uint32_t n, bool have_in) {
    for (uint32_t i = 0; i < n; i++) {
        if (hin[i + 1] < hin[i] || hout[i + 1] < hout[i] || hop[i] > FL_FEED_FINISH) return false;
        if (hin[i + 1] - hin[i] > FL_DFL_MAX_PIECE) return false;
    }
    return have_in || hin[n] <= hin[0];
}

enum fl_dfl_route_kind { FL_DFL_DRAIN = 0, FL_DFL_FINISHED = 1, FL_DFL_SKIPPED = 2, FL_DFL_ACTIVE = 3 };
struct fl_dfl_route {
    int kind = FL_DFL_SKIPPED;
    uint64_t from = 0, give = 0;             // drain: pending bytes [from, from + give) go into the slot
    int32_t status = FL_DFL_ST_NEED_INPUT;  // what the feed reports for the stream (active: once it is settled)
};

// What one feed does with a stream whose piece is `piece` bytes with `op` and whose slot is `slot` bytes.  A stream with
// output left over drains it and takes nothing (consumed 0 says the piece was not taken and goes again): NEED_OUTPUT
// while bytes are left, else NEED_INPUT or the final status of a finished stream -- and the mirror is moved on.  A
// finished stream takes nothing.  An empty MORE piece with an empty slot is skipped.  The rest take their piece.
inline fl_dfl_route fl_dfl_route_stream(fl_dfl_mirror& m, uint64_t piece, int op, uint64_t slot) {
    fl_dfl_route r;
    if (m.pend_len > m.pend_pos) {
        r.kind = FL_DFL_DRAIN;
        r.from = m.pend_pos;
        r.give = slot < m.pend_len - m.pend_pos ? slot : m.pend_len - m.pend_pos;
        m.pend_pos += r.give;
        const bool left = m.pend_pos < m.pend_len;
        r.status = left ? FL_DFL_ST_NEED_OUTPUT : (m.finished ? FL_DFL_ST_OK : FL_DFL_ST_NEED_INPUT);
        if (!left) m.pend_len = m.pend_pos = 0;
    } else if (m.finished) {
        r.kind = FL_DFL_FINISHED;
        r.status = FL_DFL_ST_OK;
    } else if (!(piece == 0 && op == FL_FEED_MORE && slot == 0)) {
        r.kind = FL_DFL_ACTIVE;
    }
    return r;
}

// k_deflater_stage's grid is (jobs, slices): a slice is 256 threads of one 16-byte unit each, and the longest job decides
inline uint32_t fl_dfl_stage_slices(uint64_t max_units) {
    const uint64_t s = (max_units + 255) / 256;
    return (uint32_t)(s < 1024 ? s : 1024);
}

// The active streams of a feed, job j being stream act[j]
struct fl_dfl_layout {
    std::vector<fl_dfl_job> jobs;
    std::vector<fl_chunk> chunks;           // a job's staged input in `win`, its output in `wout`, its blocks
    std::vector<fl_sblock> blocks, units;   // every job's blocks and checksum units, job after job
    std::vector<uint32_t> block_job, unit_job;
    uint64_t win_n = 0, out_n = 0;  // bytes of the staged input and of the output of all jobs
    uint64_t max_units = 1;         // 16-byte units of the longest staged input
    uint32_t slices = 1;            // fl_dfl_stage_slices(max_units)
};

// A job's buffer and piece are staged back to back at a 16-byte boundary, rounded up to whole 16-byte units
// (k_deflater_stage writes whole units) with 16 bytes to spare; its output bound is rounded up to 16.  src_off: a device feed reads the
// caller's buffer, a host feed (`dev` false) a staged copy of in[hin[0] .. hin[n]).
inline void fl_dfl_lay_out(const fl_dfl_mirror* mirror, const std::vector<uint32_t>& act, const uint64_t* hin, const uint8_t* hop,
                           bool dev, fl_dfl_layout& lay) {
    const uint32_t nj = (uint32_t)act.size();
    lay = fl_dfl_layout();
    lay.jobs.resize(nj);
    lay.chunks.resize(nj);
    for (uint32_t j = 0; j < nj; j++) {
        const uint32_t i = act[j];
        fl_dfl_job& jb = lay.jobs[j];
        fl_chunk& c = lay.chunks[j];
        memset(&c, 0, sizeof c);
        jb.stream = i;
        jb.bl = mirror[i].bl;
        jb.n = (uint32_t)(hin[i + 1] - hin[i]);
        jb.src_off = dev ? hin[i] : hin[i] - hin[0];
        jb.hdr = mirror[i].hdr_done ? 0u : 1u;
        jb.finish = hop[i] == FL_FEED_FINISH ? 1u : 0u;
        c.first_block = (uint32_t)lay.blocks.size();
        jb.keep = fl_dfl_blocks(jb.bl, jb.n, hop[i], lay.blocks);
        c.n_blocks = (uint32_t)lay.blocks.size() - c.first_block;
        lay.block_job.insert(lay.block_job.end(), c.n_blocks, j);
        jb.ck_first = (uint32_t)lay.units.size();
        jb.ck_n = fl_dfl_checksum_units(jb.bl, jb.n, lay.units);
        lay.unit_job.insert(lay.unit_job.end(), jb.ck_n, j);
        const uint64_t L = (uint64_t)jb.bl + jb.n;
        c.in_off = lay.win_n;
        c.in_len = (uint32_t)L;
        lay.win_n += ((L + 15) & ~15ull) + 16;
        c.out_off = lay.out_n;
        c.out_cap = fl_dfl_out_bound(jb.bl, jb.n);
        lay.out_n += (c.out_cap + 15) & ~15ull;
        c.unfinished = jb.finish ? 0u : 1u;
        if ((L + 15) / 16 > lay.max_units) lay.max_units = (L + 15) / 16;
    }
    lay.slices = fl_dfl_stage_slices(lay.max_units);
}

struct fl_dfl_settled {
    bool ok = false;              // false: the job produced more than its bound -- nothing else is set, the mirror untouched
    uint64_t give = 0, pend = 0;  // bytes of the job's output for the slot, and those behind them that are kept
    uint64_t consumed = 0;
    int32_t status = FL_DFL_ST_NEED_INPUT;
};

// What becomes of the `produced` bytes of a job whose chunk is `ck` and whose slot is `slot` bytes: the slot is filled,
// the rest is pending (NEED_OUTPUT; else the final status after FINISH, else NEED_INPUT), the piece counts as taken,
// and the mirror holds what the kernels left on the device.
inline fl_dfl_settled fl_dfl_settle(fl_dfl_mirror& m, const fl_dfl_job& jb, const fl_chunk& ck, uint64_t produced, uint64_t slot) {
    fl_dfl_settled s;
    if (produced > ck.out_cap) return s;
    s.ok = true;
    s.give = produced < slot ? produced : slot;
    s.pend = produced - s.give;
    s.consumed = jb.n;
    s.status = s.pend ? FL_DFL_ST_NEED_OUTPUT : (jb.finish ? FL_DFL_ST_OK : FL_DFL_ST_NEED_INPUT);
    if (s.pend) {
        m.pend_len = s.pend;
        m.pend_pos = 0;
    }
    m.bl = jb.keep;
    m.hdr_done = 1;
    if (jb.finish) m.finished = 1;
    return s;
}
