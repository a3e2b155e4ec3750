// dict_compress_plan.h under AddressSanitizer and UBSan, as a program of its own (tests/test_dict_compress_plan_cpu.py
// builds and runs it): random and hostile batches -- empty records, empty dictionaries, streams at and over the limit,
// slots of fewer than four bytes, every mix of kinds -- through the stream table, the pass walk, the staging layout and
// the whole-stream tables of a pass of staged streams.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../flate_amd/csrc/dict_compress_plan.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    std::mt19937_64 rng(11);
    for (int it = 0; it < 4000; it++) {
        const uint32_t n_dicts = (uint32_t)(rng() % 5), n = (uint32_t)(rng() % 40);
        std::vector<uint64_t> doff(n_dicts + 1);
        uint64_t at = rng() % 100;
        for (uint32_t d = 0; d <= n_dicts; d++) {
            doff[d] = at;
            at += rng() % 4 == 0 ? 0 : rng() % 3 == 0 ? 32768 + rng() % 9000 : rng() % 33000;
        }
        std::vector<fl_dict_ent> tab;
        fl_dict_table(doff.data(), n_dicts, tab);
        std::vector<uint32_t> of(n);
        std::vector<uint64_t> hin(n + 1), hout(n + 1);
        uint64_t ia = rng() % 50, oa = rng() % 50;
        bool too_long = false;
        const bool with_of = n_dicts != 1 || rng() % 2;
        for (uint32_t i = 0; i < n; i++) {
            of[i] = n_dicts && rng() % 4 ? (uint32_t)(rng() % n_dicts) : FL_DICT_NONE;
            const uint32_t d = with_of ? of[i] : 0u;
            const uint32_t D = d == FL_DICT_NONE ? 0u : tab[d].hist_len;
            uint64_t len = rng() % 5 == 0 ? rng() % 5 : rng() % 70000;
            if (d != FL_DICT_NONE && rng() % 20 == 0) len = 65535 - D + (rng() % 3) - 1;  // at the limit, one under, one over
            if (d != FL_DICT_NONE && rng() % 40 != 0 && D + len > 65535) len = 65535 - D;
            if (d != FL_DICT_NONE && D + len > 65535) too_long = true;
            hin[i] = ia;
            hout[i] = oa;
            ia += len;
            oa += rng() % 10 == 0 ? rng() % 6 : len + 64;
        }
        hin[n] = ia;
        hout[n] = oa;
        CHECK(fl_dictc_args_ok(0, 6, doff.data(), n_dicts, with_of ? of.data() : nullptr, with_of, n) == (with_of || n_dicts == 1));
        CHECK(!fl_dictc_args_ok(1, 6, doff.data(), n_dicts, of.data(), true, n));
        CHECK(!fl_dictc_args_ok(0, (int)(rng() % 4), doff.data(), n_dicts, of.data(), true, n));
        if (!with_of && n_dicts != 1) continue;
        std::vector<fl_dictc_stream> ds;
        const int rc = fl_dictc_streams(hin.data(), n, tab, with_of ? of.data() : nullptr, ds);
        CHECK((rc == FLATE_HIP_E_UNSUPPORTED) == too_long && (rc == 0 || rc == FLATE_HIP_E_UNSUPPORTED));
        if (rc) continue;
        CHECK(ds.size() == n);
        for (uint32_t i = 0; i < n; i++) {
            if (ds[i].dict == FL_DICT_NONE) continue;
            const fl_dict_ent& e = tab[ds[i].dict];
            CHECK(ds[i].hist == e.hist_len && ds[i].t_start >= e.start && ds[i].t_start + ds[i].hist == e.end);
        }
        std::vector<fl_chunk> chunks;
        const int mode = 4 + (int)(rng() % 6);
        CHECK(fl_chunk_table(hin.data(), hout.data(), n, 0, 0, mode, nullptr, chunks));
        fl_pass_cfg cfg;
        cfg.n_chunks = n;
        cfg.max_pass_chunks = 1 + rng() % 8;
        const uint64_t pass_bytes = 1 + rng() % 200000;
        const uint32_t pass_streams = 1 + (uint32_t)(rng() % 6);
        const int container = rng() % 2 ? 2 : 0;
        uint64_t covered = 0;
        for (uint64_t c0 = 0, k = 0; c0 < n; k++) {
            const fl_dictc_pick pk = fl_dictc_pass_next(cfg, chunks.data(), ds.data(), c0, k, mode, pass_bytes, pass_streams);
            CHECK(pk.nc >= 1 && c0 + pk.nc <= n);
            for (uint32_t i = 0; i < pk.nc; i++) CHECK(fl_dictc_kind(mode, ds[c0 + i], chunks[c0 + i].in_len) == pk.kind);
            if (pk.kind == FL_DICTC_CHUNK) CHECK(pk.nc <= cfg.max_pass_chunks);
            if (pk.kind == FL_DICTC_STAGED) {
                CHECK(pk.nc <= pass_streams);
                std::vector<fl_chunk> pass(chunks.begin() + c0, chunks.begin() + c0 + pk.nc);  // (exactly nc entries on the heap)
                std::vector<fl_dictc_stream> pds(ds.begin() + c0, ds.begin() + c0 + pk.nc);
                std::vector<fl_dictc_job> jobs;
                const uint64_t bytes = fl_dictc_stage(pass.data(), pds.data(), pk.nc, jobs);
                CHECK(jobs.size() == pk.nc);
                uint64_t end = 0;
                for (uint32_t i = 0; i < pk.nc; i++) {
                    CHECK(jobs[i].dst % 16 == 0 && jobs[i].dst >= end);
                    end = jobs[i].dst + (((uint64_t)jobs[i].n + jobs[i].hist + 15) & ~15ull);
                    CHECK(jobs[i].n + jobs[i].hist <= 65535);
                }
                CHECK(end + FL_DICTC_STAGE_TAIL <= bytes);
                fl_dictc_staged_chunks(pass.data(), jobs.data(), pk.nc, container);
                StreamTables tabs;
                std::vector<uint32_t> blk;
                const uint32_t nb = fl_dictc_pass_tables(pass.data(), jobs.data(), pk.nc, tabs, blk);
                CHECK(blk.size() == nb && tabs.tiles.size() == pk.nc && tabs.pieces.size() == pk.nc && tabs.zones.empty());
                for (uint32_t i = 0; i < pk.nc; i++) {
                    const fl_chunk& c = pass[i];
                    const fl_piece& pc = tabs.pieces[c.piece0];
                    CHECK(c.n_piece == 1 && pc.start == jobs[i].hist && pc.end == c.in_len && pc.flags == 1u);
                    CHECK(c.n_slides == 0 && c.n_flush == (jobs[i].hist ? 1u : 0u) && tabs.tiles[i].tgt0 == jobs[i].hist);
                    CHECK(c.in_off == jobs[i].dst && c.in_len == jobs[i].n + jobs[i].hist);
                    for (uint32_t s = 0; s < pc.n_seg; s++) CHECK(tabs.segs[pc.seg0 + s].h0 + FL_SEG > pc.start);
                    const uint64_t cap0 = hout[c0 + i + 1] - hout[c0 + i];
                    CHECK(c.out_off == hout[c0 + i] + (container == 2 ? 4u : 0u));
                    CHECK(c.out_cap == (container == 2 ? (cap0 >= 4 ? cap0 - 4 : 0) : cap0));
                }
                CHECK(fl_dictc_ws_bytes(bytes, pk.nc) >= bytes);
            }
            covered += pk.nc;
            c0 += pk.nc;
        }
        CHECK(covered == n);
    }
    std::puts("dict_compress_plan ok");
    return 0;
}
