// compress_impl's host-side decisions (flate_amd/csrc/pass_plan.h) over random batches, hostile ones among them: empty
// batches, offsets that do not grow, flush points beyond the input, and a batch of nearly 2^32 chunks (through the walk
// only: it needs no table when every chunk takes the chunk path).  Built with -fsanitize=address,undefined by
// tests/test_host_cpp.py; needs no GPU.  It checks that every call returns, that the passes cover [0, n) exactly once and
// that a pass's block count is the length of its block -> chunk table -- not what the calls decide
// (tests/test_compress_plan_cpu.py does).
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/csrc/pass_plan.h"

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

static fl_pass_cfg random_cfg(uint64_t n) {
    fl_pass_cfg c;
    c.n_chunks = n;
    c.host_pass_chunks = 1 + below(below(2) ? 8 : 2048);
    c.max_pass_chunks = 1 + below(below(2) ? 8 : 40000);
    c.pinned = below(2) != 0;
    c.ramp = below(2) != 0;
    c.planned = below(4) == 0;
    return c;
}

int main() {
    const int modes[] = {0, 1, 4, 6, 9};
    uint64_t tables = 0, passes_seen = 0, refused = 0;
    for (int set_no = 0; set_no < 4000; set_no++) {
        const bool hostile = set_no % 3 == 0;
        const uint32_t n = hostile && below(8) == 0 ? 0u : 1 + (uint32_t)below(below(4) ? 40 : 3000);
        const int mode = modes[below(5)];
        // ---- offsets: short and long inputs mixed, the lengths of the seam among them
        std::vector<uint64_t> hin(n + 1), hout(n + 1);
        hin[0] = below(1u << 20);
        hout[0] = below(1u << 20);
        for (uint32_t i = 0; i < n; i++) {
            uint64_t len;
            switch (below(8)) {
                case 0: len = 0; break;
                case 1: len = 65535; break;
                case 2: len = 65536; break;
                case 3: len = below(400000); break;
                default: len = below(65536); break;
            }
            hin[i + 1] = hin[i] + len;
            hout[i + 1] = hout[i] + below(1u << 18);
            if (hostile && below(16) == 0) hin[i + 1] = below(2) ? hin[i] - below(1000) : hin[i] + 0xfff00000ull + below(0x1000000);  // going back, or too long
            if (hostile && below(16) == 0) hout[i + 1] = hout[i] - below(1000);
        }
        // ---- the flush points of a flush call (one stream): ascending as the entry point demands, or anything
        const bool flush = n == 1 && below(2);
        std::vector<uint64_t> fpos;
        if (flush) {
            const uint64_t len = hin[1] - hin[0];
            uint64_t at = 0;
            for (uint64_t k = below(5); k > 0; k--) {
                at = hostile ? below(2) ? (uint32_t)rnd() % 3000000u : len + below(200000) : at + below(len - at + 1);
                fpos.push_back(at);
            }
        }
        const FlushSpec fs{fpos.data(), (uint32_t)fpos.size(), below(2) != 0};
        const FlushSpec* fsp = flush ? &fs : nullptr;
        // ---- the chunk table
        std::vector<fl_chunk> chunks;
        const uint64_t in_shift = below(2) ? hin[0] : 0, out_shift = below(2) ? hout[0] : 0;
        if (!fl_chunk_table(hin.data(), hout.data(), n, in_shift, out_shift, mode, fsp, chunks)) {
            bool long_one = false;
            for (uint32_t i = 0; i < n; i++) long_one |= hin[i + 1] - hin[i] > (mode >= 4 ? 0xfff00000ull : 0xfffffff0ull);
            CHECK(long_one);
            refused++;
            continue;
        }
        CHECK(chunks.size() == n);
        for (uint32_t i = 0; i < n; i++) {
            CHECK(chunks[i].in_len == hin[i + 1] - hin[i] && chunks[i].in_off == hin[i] - in_shift);
            CHECK(chunks[i].out_cap == hout[i + 1] - hout[i] && chunks[i].out_off == hout[i] - out_shift);
        }
        // ---- the walk and the tables of every pass
        const fl_pass_cfg cfg = random_cfg(n);
        const uint64_t stream_bytes = below(2) ? 4096ull << 20 : 1 + below(600000);
        uint64_t covered = 0, pass_index = 0, blocks = 0;
        bool all_chunk_passes = true;
        for (uint64_t c0 = 0; c0 < n; pass_index++) {
            const fl_pass_pick pk = fl_pass_next(cfg, chunks.data(), c0, pass_index, mode, flush, stream_bytes);
            CHECK(pk.nc >= 1 && c0 + pk.nc <= n);
            for (uint32_t i = 0; i < pk.nc; i++) CHECK(fl_whole_stream(mode, flush, chunks[c0 + i].in_len) == pk.stream);
            CHECK(pk.stream || pk.nc <= cfg.max_pass_chunks);
            StreamTables tabs;
            std::vector<uint32_t> blk_chunk;
            std::vector<fl_sblock> sblocks;
            const uint32_t nb = fl_pass_tables(&chunks[c0], pk.nc, pk.stream, mode, fsp, tabs, blk_chunk, sblocks);
            CHECK(nb == blk_chunk.size());
            uint32_t sum = 0;
            for (uint32_t i = 0; i < pk.nc; i++) {
                CHECK(chunks[c0 + i].first_block == sum);
                sum += chunks[c0 + i].n_blocks;
            }
            CHECK(sum == nb);
            for (size_t b = 0; b < blk_chunk.size(); b++) CHECK(blk_chunk[b] < pk.nc && (b == 0 || blk_chunk[b] >= blk_chunk[b - 1]));
            CHECK(pk.stream ? sblocks.empty() && tabs.pieces.size() >= (fsp && !fs.finish && fpos.empty() ? 0u : 1u)
                            : tabs.pieces.empty() && (fsp || sblocks.empty()));
            all_chunk_passes &= !pk.stream;
            blocks += nb;
            covered += pk.nc;
            c0 += pk.nc;
            tables++;
        }
        CHECK(covered == n);
        passes_seen += pass_index;
        if (all_chunk_passes && !flush) CHECK(blocks == fl_batch_blocks(chunks.data(), n, mode));
        // ---- two streams and the rectangle rows: whatever they say, they say it inside their arrays
        const bool two = fl_two_eligible(cfg, cfg.pinned && !cfg.planned, cfg.planned ? below(4) : 0, mode, flush, below(8) == 0, chunks.data());
        if (two) {
            for (uint32_t i = 0; i < n; i++) CHECK(chunks[i].in_len <= FLATE_HIP_MAX_LZ_CHUNK);
            fl_two_slices s;
            const bool on = fl_two_from_schedule(cfg, s);
            CHECK(on == (s.sched.size() >= 2) && s.nb == 2 * s.nc);
            uint64_t at = 0;
            for (const fl_pass& p : s.sched) {
                CHECK(p.c0 == at && p.nc >= 1 && p.nc <= s.nc);
                at += p.nc;
            }
            CHECK(at == n);
        }
        for (uint64_t c0 = 0; c0 < n; c0 += 1 + below(n)) {
            const uint32_t nc = 1 + (uint32_t)below(n - c0);
            const fl_rect r = fl_rect_rows(&hout[c0], nc, (int)below(3) - 1);
            CHECK(r.urows <= nc && (r.urows == 0 || (r.urows >= 64 && r.half >= 4096 && r.half <= r.pitch / 2 && r.half % 16 == 0)));
            for (uint32_t i = 0; i < r.urows; i++) CHECK(hout[c0 + i + 1] - hout[c0 + i] == r.pitch);
        }
    }
    // ---- nearly 2^32 chunks, all of length zero: the walk alone (no table), every pass a sub-batch
    {
        const int set_no = -1;
        for (const uint64_t n : {0xffffffffull, 0xfffffff0ull, 0x100000001ull >> 1}) {
            for (int pinned = 0; pinned < 2; pinned++) {
                fl_pass_cfg cfg;
                cfg.n_chunks = n;
                cfg.pinned = pinned != 0;
                uint64_t c0 = 0, k = 0;
                for (; c0 < n; k++) {
                    const fl_pass_pick pk = fl_pass_next(cfg, nullptr, c0, k, 6, false, 4096ull << 20);
                    CHECK(pk.nc >= 1 && !pk.stream && c0 + pk.nc <= n && pk.nc <= cfg.max_pass_chunks);
                    c0 += pk.nc;
                }
                CHECK(c0 == n && k >= n / cfg.max_pass_chunks);
                passes_seen += k;
            }
        }
        std::vector<fl_pass> sched;
        fl_pass_cfg cfg;
        cfg.n_chunks = 0;
        CHECK(fl_pass_schedule(cfg, sched) == 0 && sched.empty());
    }
    printf("ok: %llu passes with tables, %llu passes walked, %llu batches refused\n", (unsigned long long)tables,
           (unsigned long long)passes_seen, (unsigned long long)refused);
    return tables > 4000 && refused > 50 ? 0 : 2;
}
