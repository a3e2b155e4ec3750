// The host decisions of a resumable deflater's feed (flate_amd/csrc/deflater_plan.h) over hostile tables -- offsets near
// 2^64, offsets that go back, ops 3..255, pieces at the limit and one byte above it -- and over random valid sessions.
// Built with -fsanitize=address,undefined by tests/test_host_cpp.py; needs no GPU.  It checks invariants -- a table is
// accepted exactly when it ascends, knows its ops and keeps to the piece limit; every index a layout hands out is inside
// its table, the staged regions are aligned and disjoint, the blocks and units lie inside their job's staged input; every
// byte a job produced is handed out once, whatever the slots -- not what the rules decide (tests/test_deflater_cpu.py does).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/csrc/deflater_plan.h"

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

static uint64_t tables_seen = 0, tables_refused = 0, feeds_seen = 0, jobs_seen = 0, drains_seen = 0;

// every invariant of one layout; `dev`: src_off is the caller's offset
static int check_layout(int set_no, const std::vector<fl_dfl_mirror>& mir, const std::vector<uint32_t>& act, const std::vector<uint64_t>& hin,
                        const std::vector<uint8_t>& hop, bool dev, const fl_dfl_layout& lay) {
    const size_t nj = act.size();
    CHECK(lay.jobs.size() == nj && lay.chunks.size() == nj);
    CHECK(lay.block_job.size() == lay.blocks.size() && lay.unit_job.size() == lay.units.size());
    uint64_t in_end = 0, out_end = 0, nb = 0, nck = 0, units_max = 1;
    for (size_t j = 0; j < nj; j++) {
        const fl_dfl_job& jb = lay.jobs[j];
        const fl_chunk& c = lay.chunks[j];
        const uint32_t i = act[j];
        const uint64_t L = (uint64_t)jb.bl + jb.n;
        CHECK(jb.stream == i && jb.bl == mir[i].bl && jb.n == hin[i + 1] - hin[i] && c.in_len == L);
        CHECK(jb.src_off == (dev ? hin[i] : hin[i] - hin[0]) && (dev || jb.src_off + jb.n <= hin.back() - hin[0]));
        CHECK(jb.hdr == (mir[i].hdr_done ? 0u : 1u) && jb.finish == (hop[i] == FL_FEED_FINISH ? 1u : 0u) && c.unfinished == 1 - jb.finish);
        CHECK((c.in_off & 15) == 0 && (c.out_off & 15) == 0 && c.in_off >= in_end && c.out_off >= out_end);
        in_end = c.in_off + ((L + 15) & ~15ull) + 16;  // whole units and 16 bytes to spare
        out_end = c.out_off + c.out_cap;
        CHECK(in_end <= lay.win_n && out_end <= lay.out_n && c.out_cap == fl_dfl_out_bound(jb.bl, jb.n));
        CHECK(c.first_block == nb && (uint64_t)c.first_block + c.n_blocks <= lay.blocks.size());
        uint64_t covered = 0;
        for (uint32_t k = 0; k < c.n_blocks; k++) {
            const fl_sblock& b = lay.blocks[c.first_block + k];
            CHECK(lay.block_job[c.first_block + k] == j && b.len <= FL_BLOCK_BYTES && (uint64_t)b.start + b.len <= L);
            if (!(b.flags & 2)) CHECK(b.start == covered);
            covered += b.len;
        }
        CHECK(covered + jb.keep == L && jb.keep < FL_BLOCK_BYTES && (hop[i] == FL_FEED_MORE || jb.keep == 0));
        nb += c.n_blocks;
        CHECK(jb.ck_first == nck && (uint64_t)jb.ck_first + jb.ck_n <= lay.units.size());
        uint64_t at = jb.bl;
        for (uint32_t k = 0; k < jb.ck_n; k++) {
            const fl_sblock& u = lay.units[jb.ck_first + k];
            CHECK(lay.unit_job[jb.ck_first + k] == j && u.start == at && u.len >= 1 && u.len <= FL_BLOCK_BYTES);
            at += u.len;
        }
        CHECK(at == L);
        nck += jb.ck_n;
        units_max = std::max(units_max, (L + 15) / 16);
    }
    CHECK(nb == lay.blocks.size() && nck == lay.units.size());
    CHECK(lay.max_units == units_max && lay.slices == fl_dfl_stage_slices(units_max) && lay.slices >= 1 && lay.slices <= 1024);
    CHECK((uint64_t)lay.slices * 256 >= std::min<uint64_t>(units_max, 1024 * 256));
    jobs_seen += nj;
    return 0;
}

// ---- hostile tables: what is accepted is what may be laid out
static int walk_hostile(int set_no) {
    const uint32_t n = (uint32_t)below(6) + 1;
    const int hostile = (int)below(8);  // 0..2: a good table
    const uint32_t victim = (uint32_t)below(n);
    std::vector<uint64_t> hin(n + 1ull), hout(n + 1ull);
    std::vector<uint8_t> hop(n);
    const uint64_t room = (uint64_t)n * FL_DFL_MAX_PIECE + n;
    hin[0] = below(4) ? below(1ull << 40) : ~0ull - room - below(1000);  // (near 2^64: the offsets still ascend)
    hout[0] = below(4) ? below(1ull << 40) : ~0ull - below(1ull << 30) - (1ull << 32);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t piece = below(8) ? below(200000) : 0;
        if (i == victim && hostile == 1) piece = FL_DFL_MAX_PIECE;      // at the limit: good
        if (i == victim && hostile == 3) piece = FL_DFL_MAX_PIECE + 1;  // one above
        hin[i + 1] = hin[i] + piece;
        hout[i + 1] = hout[i] + below(1ull << 28);
        hop[i] = (uint8_t)below(3);
    }
    if (hostile == 4) hop[victim] = (uint8_t)(3 + below(253));
    if (hostile == 5) hin[victim + 1] = hin[victim] - 1 - below(hin[victim] + 1);   // goes back, by one or to the bottom
    if (hostile == 6) hout[victim + 1] = hout[victim] - 1 - below(hout[victim] + 1);
    if (hostile == 7) hin[victim + 1] = hin[victim] + (1ull << 63) + below(1ull << 62);  // (wraps: the next one goes back, or the piece is too long)
    const bool have_in = below(4) != 0;
    bool good = true;
    for (uint32_t i = 0; i < n; i++)
        good = good && hin[i + 1] >= hin[i] && hout[i + 1] >= hout[i] && hop[i] <= 2 && hin[i + 1] - hin[i] <= FL_DFL_MAX_PIECE;
    good = good && (have_in || hin[n] == hin[0]);
    const bool ok = fl_dfl_feed_ok(hin.data(), hout.data(), hop.data(), n, have_in);
    tables_seen++;
    CHECK(ok == good);
    if (hostile >= 3) CHECK(!ok);
    if (!ok) {
        tables_refused++;
        return 0;
    }
    // an accepted table is laid out as it stands, the longest piece behind a buffer that is as full as it gets
    std::vector<fl_dfl_mirror> mir(n);
    std::vector<uint32_t> act;
    for (uint32_t i = 0; i < n; i++) {
        mir[i].bl = below(2) ? FL_BLOCK_BYTES - 1 : (uint32_t)below(FL_BLOCK_BYTES);
        mir[i].hdr_done = (uint8_t)below(2);
        if (fl_dfl_route_stream(mir[i], hin[i + 1] - hin[i], hop[i], hout[i + 1] - hout[i]).kind == FL_DFL_ACTIVE) act.push_back(i);
    }
    fl_dfl_layout lay;
    const bool dev = below(2);
    fl_dfl_lay_out(mir.data(), act, hin.data(), hop.data(), dev, lay);
    return check_layout(set_no, mir, act, hin, hop, dev, lay);
}

// ---- a random valid session: feeds until every stream is finished and drained
static int walk_session(int set_no) {
    const uint32_t n = (uint32_t)below(8) + 1;
    std::vector<fl_dfl_mirror> mir(n);
    std::vector<uint64_t> made(n, 0), got(n, 0), pend_from(n, 0);  // bytes produced, handed out; where the pending ones start
    std::vector<uint32_t> left(n);                                // feeds until the stream finishes
    for (uint32_t i = 0; i < n; i++) left[i] = (uint32_t)below(6);
    const uint64_t slots[] = {0, 1, 7, 258, 70000, 1ull << 22};
    for (int feed = 0; feed < 100000; feed++) {
        bool all_done = true;
        for (uint32_t i = 0; i < n; i++) all_done = all_done && mir[i].finished && mir[i].pend_len == 0;
        if (all_done) break;
        CHECK(feed < 99999);
        std::vector<uint64_t> hin(n + 1ull), hout(n + 1ull);
        std::vector<uint8_t> hop(n);
        hin[0] = below(1ull << 40);
        hout[0] = below(1ull << 40);
        for (uint32_t i = 0; i < n; i++) {
            hin[i + 1] = hin[i] + (below(3) ? below(3 * FL_BLOCK_BYTES) : below(20));
            hout[i + 1] = hout[i] + slots[below(6)];
            hop[i] = left[i] == 0 ? FL_FEED_FINISH : (uint8_t)below(2);
        }
        CHECK(fl_dfl_feed_ok(hin.data(), hout.data(), hop.data(), n, true));
        std::vector<uint32_t> act;
        for (uint32_t i = 0; i < n; i++) {
            const fl_dfl_mirror was = mir[i];
            const uint64_t slot = hout[i + 1] - hout[i];
            const fl_dfl_route r = fl_dfl_route_stream(mir[i], hin[i + 1] - hin[i], hop[i], slot);
            CHECK(r.give <= slot && mir[i].pend_pos <= mir[i].pend_len);
            if (r.kind == FL_DFL_DRAIN) {
                CHECK(r.from == was.pend_pos && r.from + r.give <= was.pend_len && pend_from[i] + r.from == got[i]);
                got[i] += r.give;
                drains_seen++;
            } else {
                CHECK(r.give == 0 && was.pend_len == was.pend_pos);
            }
            if (r.kind == FL_DFL_ACTIVE) {
                CHECK(!was.finished);
                act.push_back(i);
            }
        }
        fl_dfl_layout lay;
        const bool dev = below(2);
        fl_dfl_lay_out(mir.data(), act, hin.data(), hop.data(), dev, lay);
        if (check_layout(set_no, mir, act, hin, hop, dev, lay)) return 1;
        for (size_t j = 0; j < act.size(); j++) {
            const uint32_t i = act[j];
            const fl_chunk& ck = lay.chunks[j];
            const uint64_t slot = hout[i + 1] - hout[i];
            fl_dfl_mirror m = mir[i];
            CHECK(!fl_dfl_settle(m, lay.jobs[j], ck, ck.out_cap + 1 + below(1000), slot).ok && m.bl == mir[i].bl && m.pend_len == 0);
            const uint64_t p = below(4) ? below(ck.out_cap + 1) : (below(2) ? 0 : ck.out_cap);
            const fl_dfl_settled s = fl_dfl_settle(mir[i], lay.jobs[j], ck, p, slot);
            CHECK(s.ok && s.give <= slot && s.give + s.pend == p && s.consumed == lay.jobs[j].n);
            CHECK(mir[i].pend_len == s.pend && mir[i].pend_pos == 0 && mir[i].bl == lay.jobs[j].keep && mir[i].hdr_done == 1);
            CHECK(made[i] == got[i]);  // (nothing was pending when the stream took its piece)
            pend_from[i] = made[i] + s.give;
            made[i] += p;
            got[i] += s.give;
            if (left[i]) left[i]--;
        }
        feeds_seen++;
    }
    for (uint32_t i = 0; i < n; i++) CHECK(got[i] == made[i]);
    return 0;
}

int main() {
    for (int set_no = 0; set_no < 400; set_no++)
        if (walk_hostile(set_no)) return 1;
    for (int set_no = 0; set_no < 300; set_no++)
        if (walk_session(set_no)) return 1;
    if (tables_refused == 0 || tables_refused == tables_seen || drains_seen == 0) {
        printf("no mix: %llu of %llu tables refused, %llu drains\n", (unsigned long long)tables_refused, (unsigned long long)tables_seen,
               (unsigned long long)drains_seen);
        return 1;
    }
    printf("ok: %llu tables (%llu refused), %llu feeds, %llu jobs, %llu drains\n", (unsigned long long)tables_seen,
           (unsigned long long)tables_refused, (unsigned long long)feeds_seen, (unsigned long long)jobs_seen, (unsigned long long)drains_seen);
    return 0;
}
