// The host decisions of the inflate entry points (flate_amd/csrc/inflate_plan.h) and of flate_hip_decompress_members
// (flate_amd/csrc/member_plan.h, the host's side) over random inputs, hostile ones among them: empty streams, streams at and
// beyond the length limit, counts up to 2^32 - 1, member tables with empty streams, starts that go backwards or lie beyond
// their stream.  Built with -fsanitize=address,undefined by tests/test_host_cpp.py; needs no GPU.  It checks invariants --
// the sub-batches partition [0, n), the members a table is accepted with are a contiguous ascending cover of the input
// range and of the slots, a table's capacity is never below what it holds, every index handed out is inside its array --
// not what the rules decide (tests/test_inflate_plan_cpu.py and tests/test_members_cpu.py do).  The resumable inflater's host
// feeds are walked too: tables that go back, slots around the least one, and the rebased tables of those that are accepted.
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/csrc/inflate_plan.h"
#include "../../flate_amd/csrc/member_plan.h"

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

static uint64_t batches_seen = 0, tables_seen = 0, tables_refused = 0;

// a stream length: mostly small, now and then empty, at the limit or beyond it
static uint64_t a_length() {
    switch (below(16)) {
        case 0: return 0;
        case 1: return FL_INF_MAX_IN_BYTES - below(2);
        case 2: return FL_INF_MAX_IN_BYTES + 1 + below(1000);
        case 3: return below(1ull << 33);
        default: return below(100000);
    }
}

// ---- sub-batches, ring, pinned rule: any count, any knob
static int walk_counts(int set_no) {
    const uint32_t ns[] = {1, 2, 8, 9, 20, 4096, 4097, 6145, 6146, 16385, 0x7fffffffu, 0xfffffffeu, 0xffffffffu, (uint32_t)below(1u << 20) + 1,
                           (uint32_t)rnd() | 1u};
    const size_t knobs[] = {1, 2, 3, 1024, 4096, (size_t)below(100000) + 1, 0x7fffffff};
    for (uint32_t n : ns)
        for (size_t knob : knobs) {
            const uint32_t sub = fl_inflate_sub_batch(n, knob);
            CHECK(sub >= 1 && sub <= n);
            // the driver's loop: c0 += sub while c0 < n -- the pieces partition [0, n), none is empty, all but the last are equal
            const uint64_t pieces = ((uint64_t)n + sub - 1) / sub;
            CHECK((pieces - 1) * sub < n && pieces * sub >= n);
            const uint64_t last = n - (pieces - 1) * sub;
            CHECK(last >= 1 && last <= sub);
            if (pieces <= 64) {
                uint64_t c0 = 0, seen = 0;
                for (; c0 < n; c0 += sub) seen += std::min<uint64_t>(sub, n - c0);
                CHECK(seen == n);
            }
            (void)fl_inflate_ring_large((int64_t)rnd(), n);
            (void)fl_inflate_ring_large(-1, n);
            (void)fl_inflate_pin_io(below(2), below(2), rnd(), rnd(), n, knob);
            (void)fl_inflate_pool_release(rnd());
        }
    return 0;
}

// ---- a batch: chunk table, the par rule, the copy-out plan
static int walk_batch(int set_no) {
    const uint32_t n = (uint32_t)below(below(8) ? 40 : 3000);
    std::vector<uint64_t> hin(n + 1ull), hout(n + 1ull), out_len(n);
    hin[0] = below(1ull << 40);
    hout[0] = below(1ull << 40);
    for (uint32_t i = 0; i < n; i++) {
        hin[i + 1] = hin[i] + a_length();
        hout[i + 1] = hout[i] + (below(4) ? below(1ull << 20) : below(3) ? 0 : below(1ull << 36));
        out_len[i] = below(3) ? below(hout[i + 1] - hout[i] + 1) : 0;
    }
    const bool shifted = below(2);
    std::vector<fl_chunk> chunks;
    const uint32_t bad = fl_inflate_oversize(hin.data(), n);
    CHECK(bad <= n);
    const bool ok = fl_inflate_chunks(hin.data(), below(4) ? hout.data() : nullptr, n, shifted ? hin[0] : 0, shifted ? hout[0] : 0, chunks);
    CHECK(ok == (bad == n));
    if (bad < n) CHECK(hin[bad + 1] - hin[bad] > FL_INF_MAX_IN_BYTES);
    for (uint32_t i = 0; i < bad; i++) CHECK(hin[i + 1] - hin[i] <= FL_INF_MAX_IN_BYTES);
    if (ok) {
        CHECK(chunks.size() == n);
        for (uint32_t i = 0; i < n; i++) {
            CHECK(chunks[i].in_off + chunks[i].in_len == hin[i + 1] - (shifted ? hin[0] : 0));  // contiguous, inside the staged range
            CHECK(chunks[i].skip == 0 && chunks[i].n_blocks == 0);
            chunks[i].skip = below(5) == 0;
        }
        const int64_t knobs[] = {-1, 0, 1, 1000, 32768, 0xffffffffll};
        for (int64_t knob : knobs) {
            const fl_inflate_par p = fl_inflate_par_plan(chunks.data(), n, knob, (int)below(4));
            CHECK(p.n_big <= n && p.taken <= n);
            CHECK(!p.use || (p.min_bytes && p.n_big >= 1 && p.n_big <= FL_INF_PAR_MAX_BIG));
            CHECK(p.use || p.taken == 0);
        }
    }
    const fl_copy_out c = fl_copy_out_plan(hout.data(), out_len.data(), n);
    CHECK(c.kind == FL_COPY_OUT_NONE || c.kind == FL_COPY_OUT_DENSE || c.kind == FL_COPY_OUT_PACKED);
    if (c.kind != FL_COPY_OUT_NONE) CHECK(c.total > 0 && c.total <= hout[n] - hout[0]);
    if (c.kind == FL_COPY_OUT_DENSE) CHECK(c.end > hout[0] && c.end <= hout[n]);  // the copy stays inside the slots
    batches_seen++;
    return 0;
}

// ---- a call's member tables: capacities, then a table as a device could hand it back, good or hostile
static int walk_members(int set_no) {
    const uint32_t n = (uint32_t)below(30) + 1;
    const int container = (int)below(3);
    const uint32_t least = fl_member_least_bytes(container);
    std::vector<uint64_t> hin(n + 1ull), vin(n + 1ull), vout(n + 1ull), toff(n + 1ull), doff(n + 1ull);
    hin[0] = below(1ull << 40);
    vout[0] = below(1000);
    for (uint32_t i = 0; i < n; i++) {
        hin[i + 1] = hin[i] + (below(8) ? below(5000) : below(2) ? 0 : FL_INF_MAX_IN_BYTES);
        vout[i + 1] = vout[i] + below(100000);
    }
    for (uint32_t i = 0; i <= n; i++) vin[i] = hin[i] - hin[0];
    const uint64_t cap = fl_member_walk_offsets(hin.data(), n, container, toff.data());
    CHECK(toff[0] == 0 && toff[n] == cap);
    for (uint32_t i = 0; i < n; i++)  // what a stream can hold: len / least members, one failing one more, its remainder
        CHECK(toff[i + 1] - toff[i] >= (hin[i + 1] - hin[i]) / least + 2);
    const uint64_t n_cand = below(1000);
    CHECK(fl_member_scan_cap(n_cand, n) >= n_cand + n);
    fl_member_tiles t;
    const uint64_t base = (1ull << 44) + below(64), lo = below(1000), hi = lo + below(1ull << 34);
    if (fl_member_scan_tiles(base, lo, hi, t)) {
        CHECK(t.rel0 <= (int64_t)lo && (int64_t)lo - t.rel0 < 16 && ((base + (uint64_t)t.rel0) & 15) == 0);
        CHECK(t.rel0 + (int64_t)(t.n_tiles * FL_MEM_SCAN_TILE) >= (int64_t)hi);  // the tiles reach the last byte
        CHECK(hi == lo || t.rel0 + (int64_t)((t.n_tiles - 1) * FL_MEM_SCAN_TILE) < (int64_t)hi);
    }
    // the table: m members per stream (within what the capacity allows, small here), starts ascending from 0
    const int hostile = (int)below(6);  // 0, 1: a good table
    const uint32_t victim = (uint32_t)below(n);
    std::vector<uint32_t> mstart;
    std::vector<uint64_t> msize;
    for (uint32_t i = 0; i < n; i++) {
        doff[i] = mstart.size();
        const uint64_t len = vin[i + 1] - vin[i];
        uint32_t m = (uint32_t)std::min<uint64_t>(below(6) + 1, toff[i + 1] - toff[i]);
        if (hostile == 2 && i == victim) m = 0;
        uint64_t at = 0;
        for (uint32_t k = 0; k < m; k++) {
            if (k) at = std::min<uint64_t>(len, at + below(len / m + 1));
            mstart.push_back((uint32_t)std::min<uint64_t>(at, 0xffffffffu));
            msize.push_back(below(4) ? below(50000) : rnd());
        }
        if (i != victim || m == 0) continue;
        uint32_t* s = mstart.data() + doff[i];
        if (hostile == 3) s[0] = 1 + (uint32_t)below(100);
        if (hostile == 4 && m >= 2) { s[m - 1] = s[m - 2] + 1; s[m - 2] = s[m - 1] + 1 + (uint32_t)below(5); }
        if (hostile == 5) s[m - 1] = (uint32_t)std::min<uint64_t>(len + 1 + below(1000), 0xffffffffu);
    }
    doff[n] = mstart.size();
    const uint64_t M = doff[n];
    mstart.push_back(0xdeadbeefu);  // (behind the table: never looked at)
    msize.push_back(~0ull);
    CHECK(fl_member_count_ok(M, n, cap) == (M >= n && M <= cap));
    CHECK(!fl_member_count_ok(n - 1ull, n, cap) && !fl_member_count_ok(cap + 1, n, cap));
    std::vector<uint64_t> min_(M + 1), mout(M + 1);
    const fl_member_verdict v = fl_member_partition(doff.data(), mstart.data(), msize.data(), vin.data(), vout.data(), n, min_.data(), mout.data());
    tables_seen++;
    if (v.fault != FL_MEM_TAB_OK) {
        tables_refused++;
        CHECK(v.stream < n && (v.fault == FL_MEM_TAB_NO_FIRST || v.fault == FL_MEM_TAB_ORDER));
        CHECK(hostile >= 2 && v.stream == victim);
        return 0;
    }
    CHECK(hostile < 2 || hostile == 4 || hostile == 5);  // (4 with one member and 5 with a start above 2^32 - 1 cut short change nothing)
    CHECK(M <= cap);
    // a contiguous ascending cover of the input range and of the slots
    CHECK(min_[0] == vin[0] && min_[M] == vin[n] && mout[0] == vout[0] && mout[M] == vout[n]);
    for (uint64_t k = 0; k < M; k++) CHECK(min_[k] <= min_[k + 1] && mout[k] <= mout[k + 1]);
    for (uint32_t i = 0; i < n; i++) {
        CHECK(min_[doff[i]] == vin[i] && mout[doff[i]] == vout[i]);  // a stream's first member starts the stream and its slot
        for (uint64_t k = doff[i]; k < doff[i + 1]; k++) CHECK(min_[k] <= vin[i + 1] && mout[k] <= vout[i + 1]);
    }
    return 0;
}

// ---- a host feed of the resumable inflater: tables that ascend or go back, slots around the least one
static int walk_inflater_feed(int set_no) {
    const uint32_t n = (uint32_t)below(40);
    std::vector<uint64_t> in_off(n + 1ull), out_off(n + 1ull), hin, hout;
    std::vector<uint8_t> fin(n + 1ull);
    in_off[0] = below(2) ? below(1ull << 40) : ~0ull - (1ull << 30);
    out_off[0] = below(2) ? below(1ull << 40) : ~0ull - (1ull << 30);
    bool good = true;
    for (uint32_t i = 0; i < n; i++) {
        const uint64_t piece = below(3) ? below(100000) : 0, slot = below(3) ? FL_INFLATER_MIN_SLOT + below(100000) : below(8) ? 0 : 1 + below(257);
        in_off[i + 1] = below(50) ? in_off[i] + piece : in_off[i] - 1 - below(1000);
        out_off[i + 1] = below(50) ? out_off[i] + slot : out_off[i] - 1 - below(1000);
        fin[i] = (uint8_t)below(2);
        const uint64_t s = out_off[i + 1] - out_off[i];
        good = good && in_off[i + 1] >= in_off[i] && out_off[i + 1] >= out_off[i] && (s == 0 || s >= FL_INFLATER_MIN_SLOT);
    }
    CHECK(fl_inflater_slots_ok(in_off.data(), out_off.data(), fin.data(), n) == good);
    CHECK(fl_inflater_copy_each(n) == (n <= 16));
    if (!good) return 0;
    fl_inflater_rebase(in_off.data(), out_off.data(), n, hin, hout);
    CHECK(hin.size() == n + 1ull && hout.size() == n + 1ull && hin[0] == 0 && hout[0] == 0);
    for (uint32_t i = 0; i < n; i++)  // the same pieces and slots, inside the staged copies
        CHECK(hin[i + 1] - hin[i] == in_off[i + 1] - in_off[i] && hout[i + 1] - hout[i] == out_off[i + 1] - out_off[i] &&
              hin[i + 1] <= in_off[n] - in_off[0] && hout[i + 1] <= out_off[n] - out_off[0]);
    return 0;
}

int main() {
    for (int set_no = 0; set_no < 40; set_no++)
        if (walk_counts(set_no)) return 1;
    for (int set_no = 0; set_no < 3000; set_no++)
        if (walk_batch(set_no) || walk_members(set_no) || walk_inflater_feed(set_no)) return 1;
    if (tables_refused == 0 || tables_refused == tables_seen) {
        printf("no mix of good and hostile tables: %llu of %llu refused\n", (unsigned long long)tables_refused, (unsigned long long)tables_seen);
        return 1;
    }
    printf("ok: %llu batches, %llu member tables (%llu refused)\n", (unsigned long long)batches_seen, (unsigned long long)tables_seen,
           (unsigned long long)tables_refused);
    return 0;
}
