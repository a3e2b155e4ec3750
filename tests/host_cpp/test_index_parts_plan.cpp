// index_parts_plan.h under AddressSanitizer and UBSan, as a program of its own (tests/test_index_parts_host_cpp.py builds
// and runs it): a few thousand truncated, bit-flipped and field-mutated version-2 blobs through the validator -- each is
// refused, or accepted with every invariant the part decoder relies on true -- and hostile range lists (begins near
// 2^64, begin + len past it, slots too small) through the cutter and the part table.  Every blob lies in a heap array of
// exactly its size, so one byte read beyond it is seen.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../flate_amd/csrc/index_parts_plan.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// a table as flate_hip_compress_joined_indexed leaves it: random streams, a part of them failed, the points of the others
// by the rule over their pieces, the pieces at random places
static void random_tab(std::mt19937_64& rng, fl_idx_tab& t) {
    t = fl_idx_tab();
    t.container = (uint32_t)(rng() % 3);
    const uint64_t spacings[] = {1, 3, 1000, 65535, 1u << 20};
    t.spacing = spacings[rng() % 5];
    const uint32_t ns = (uint32_t)(rng() % 6);
    for (uint32_t i = 0; i < ns; i++) {
        fl_idx_stream s{};
        s.point0 = t.points.size();
        if (rng() % 4 == 0) {
            s.in_len = rng() % 100;
            s.status = rng() % 2 ? 100 : 102;
        } else {
            const uint32_t pieces[] = {1, 7, 1001, 65535};
            const uint32_t piece = pieces[rng() % 4];
            s.size = rng() % 3 == 0 ? rng() % 3 : rng() % (12 * (uint64_t)piece);
            std::vector<uint64_t> which, place;
            fl_idxp_point_pieces(s.size, piece, t.spacing, which);
            uint64_t at = rng() % 11;
            for (size_t q = 0; q < which.size(); q++) {
                place.push_back(at);
                at += 1 + rng() % 40;
            }
            fl_idxp_points(which.data(), place.data(), which.size(), piece, t.points);
            s.n_points = which.size();
            s.in_len = at + rng() % 20;
        }
        t.streams.push_back(s);
    }
}

// what fl_idxp_blob_parse promises of a blob it accepts
static bool invariants(const fl_idx_tab& t, uint64_t bytes) {
    if (t.container > 2 || t.spacing == 0 || t.win_bytes != 0) return false;
    if (bytes != FL_IDX_HDR_BYTES + (uint64_t)FL_IDX_STREAM_BYTES * t.streams.size() + (uint64_t)FL_IDX_POINT_BYTES * t.points.size()) return false;
    uint64_t at = 0;
    for (const fl_idx_stream& s : t.streams) {
        if (s.point0 != at || s.n_points > t.points.size() - at || s.in_len > FL_IDX_MAX_IN_LEN) return false;
        if (s.status != 0 && (s.n_points || s.size)) return false;
        if (s.status == 0 && (s.n_points < 1 || s.n_points - 1 > s.size / t.spacing)) return false;
        for (uint64_t k = 0; k < s.n_points; k++) {
            const fl_idx_point& p = t.points[at + k];
            if (p.win_off != 0 || p.in_bit >= s.in_len * 8 || p.out_pos > s.size) return false;
            if (k == 0 ? p.out_pos != 0 : (p.out_pos <= t.points[at + k - 1].out_pos || p.in_bit <= t.points[at + k - 1].in_bit)) return false;
        }
        at += s.n_points;
    }
    return at == t.points.size();
}

// a call's part table against the definition: the parts of every range tile its clipped bytes in order, each starts at
// or behind its point and ends at or before the next, at most the first and the last are not direct, and what a part
// decodes, reads and needs of scratch stays inside the stream, its input and the pass
static int check_call(const fl_idx_tab& t, const std::vector<uint32_t>& rs, const std::vector<uint64_t>& rb, const std::vector<uint64_t>& rl,
                      const std::vector<uint64_t>& off, uint64_t budget) {
    const uint32_t n = (uint32_t)rs.size();
    fl_idxp_call c;
    CHECK(fl_idxp_plan_call(t, n, rs.data(), rb.data(), rl.data(), off.data(), budget, c));
    CHECK(c.ranges.size() == n && c.slot_off.size() == c.parts.size());
    uint64_t at = 0;
    for (uint32_t j = 0; j < n; j++) {
        const fl_idx_stream& s = t.streams[rs[j]];
        const fl_idxp_range& r = c.ranges[j];
        const uint64_t cap = off[j + 1] - off[j], lp = fl_idx_clip(rb[j], rl[j], s.size);
        if (s.status != 0) {
            CHECK(r.n_parts == 0 && r.status == s.status && r.len == 0);
        } else if (lp > cap) {
            CHECK(r.n_parts == 0 && r.status == 100 && r.len == 0);
        } else if (lp == 0) {
            CHECK(r.n_parts == 0 && r.status == 0 && r.len == 0);
        } else {
            CHECK(r.status == 0 && r.len == lp && r.n_parts >= 1 && r.part0 == at && r.n_parts <= c.parts.size() - at);
            uint64_t done = 0, scratch_parts = 0;
            for (uint64_t k = 0; k < r.n_parts; k++) {
                const fl_idxp_part& p = c.parts[at + k];
                CHECK(p.range == j && p.len > 0 && p.dst == done && p.point >= s.point0 && p.point < s.point0 + s.n_points);
                CHECK(k == 0 || p.point == c.parts[at + k - 1].point + 1);
                const fl_idx_point& pt = t.points[p.point];
                const bool more = p.point + 1 < s.point0 + s.n_points;
                const uint64_t next = more ? t.points[p.point + 1].out_pos : s.size;
                CHECK(pt.out_pos + p.skip == rb[j] + done && pt.out_pos + p.skip + p.len <= next);
                CHECK(p.direct == (p.skip == 0 && pt.out_pos + p.len == next ? 1u : 0u));
                CHECK(p.direct || k == 0 || k + 1 == r.n_parts);
                CHECK(p.in_lo == pt.in_bit >> 3 && p.in_lo < p.in_hi && p.in_hi <= s.in_len);
                CHECK(!more || p.in_hi > t.points[p.point + 1].in_bit >> 3 || p.in_hi == s.in_len);
                const uint64_t slot = fl_idxp_part_scratch(p);
                CHECK(p.direct ? slot == 0 : (slot % FL_IDX_SLOT_ALIGN == 0 && slot >= p.skip + p.len + FL_IDX_SLACK));
                CHECK(c.slot_off[at + k] <= c.scratch && slot <= c.scratch - c.slot_off[at + k]);
                scratch_parts += !p.direct;
                done += p.len;
            }
            CHECK(done == lp && done <= cap && scratch_parts <= 2);
            at += r.n_parts;
        }
    }
    CHECK(at == c.parts.size() && c.n_direct + c.n_scratch == c.parts.size());
    // the passes: boundaries ascend and cover the parts; a pass stays under the budget unless it is one scratch part alone
    if (c.parts.empty()) {
        CHECK(c.scratch == 0);
    } else {
        CHECK(c.pass_first.size() >= 2 && c.pass_first.front() == 0 && c.pass_first.back() == c.parts.size());
        for (size_t k = 0; k + 1 < c.pass_first.size(); k++) {
            CHECK(c.pass_first[k] < c.pass_first[k + 1]);
            uint64_t used = 0, ns = 0;
            for (uint64_t q = c.pass_first[k]; q < c.pass_first[k + 1]; q++) {
                CHECK(c.slot_off[q] == used);
                used += fl_idxp_part_scratch(c.parts[q]);
                ns += !c.parts[q].direct;
            }
            CHECK(used <= budget || ns == 1);
        }
    }
    return 0;
}

int main() {
    std::mt19937_64 rng(43);
    uint64_t accepted = 0, refused = 0, parts_seen = 0;
    for (int it = 0; it < 400; it++) {
        fl_idx_tab t;
        random_tab(rng, t);
        const uint64_t n = fl_idxp_blob_bytes(t);
        uint8_t* good = (uint8_t*)std::malloc(n);
        CHECK(good);
        CHECK(fl_idxp_blob_write(t, good) == n && fl_idxp_blob_version(good, n) == FL_IDXP_VERSION);
        fl_idx_tab back;
        CHECK(fl_idxp_blob_parse(good, n, back) && invariants(back, n));
        CHECK(back.streams.size() == t.streams.size() && back.points.size() == t.points.size() && back.container == t.container &&
              back.spacing == t.spacing);
        for (size_t k = 0; k < t.points.size(); k++)
            CHECK(back.points[k].in_bit == t.points[k].in_bit && back.points[k].out_pos == t.points[k].out_pos);
        {  // the version-1 parser refuses it
            fl_idx_tab v1;
            uint64_t wa = 0;
            CHECK(!fl_idx_blob_parse(good, n, v1, &wa));
        }
        // ---- mutants: each in an array of exactly its size
        for (int m = 0; m < 12; m++) {
            uint64_t len = n;
            const int kind = (int)(rng() % 5);
            if (kind == 0) len = rng() % (n + 1);                  // truncated
            if (kind == 1 && rng() % 2) len = n + 1 + rng() % 40;  // something behind it
            uint8_t* mut = (uint8_t*)std::malloc(len ? len : 1);
            CHECK(mut);
            for (uint64_t b = 0; b < len; b++) mut[b] = b < n ? good[b] : (uint8_t)rng();
            if (kind == 2 && len) {  // bits flipped
                for (int f = 0, nf = 1 + (int)(rng() % 3); f < nf; f++) mut[rng() % len] ^= (uint8_t)(1u << (rng() % 8));
            }
            if (kind == 3 && len >= 8) {  // a field replaced: a small number, a huge one, one near a power of two
                const uint64_t field = (rng() % (len / 8)) * 8;
                const uint64_t vals[] = {0, 1, rng() % 100, ~0ull, ~0ull - rng() % 100, 1ull << 32, (1ull << 63) + rng() % 3, rng()};
                fl_idx_put64(mut + field, vals[rng() % 8]);
            }
            if (kind == 4 && len >= 48) {  // a window: win_bytes, or the window length of a point
                const uint64_t np = t.points.size();
                if (np && rng() % 2) {
                    const uint64_t at = FL_IDX_HDR_BYTES + (uint64_t)FL_IDX_STREAM_BYTES * t.streams.size() + FL_IDX_POINT_BYTES * (rng() % np) + 16;
                    fl_idx_put32(mut + at, 1 + (uint32_t)(rng() % 32768));
                } else {
                    fl_idx_put64(mut + 32, 1 + rng() % 70000);
                }
                fl_idx_tab got;
                CHECK(!fl_idxp_blob_parse(mut, len, got));
            }
            fl_idx_tab got;
            if (fl_idxp_blob_parse(len ? mut : nullptr, len, got)) {
                CHECK(invariants(got, len));
                // (what was accepted is cut as what was written is)
                if (!got.streams.empty()) {
                    std::vector<uint32_t> rs(1, (uint32_t)(rng() % got.streams.size()));
                    std::vector<uint64_t> rb(1, rng() % 3 ? 0 : rng()), rl(1, ~0ull), off = {0, ~0ull};
                    if (check_call(got, rs, rb, rl, off, 1 + rng() % 100000)) return 1;
                }
                accepted++;
            } else {
                refused++;
            }
            std::free(mut);
        }
        // ---- hostile ranges against the good table
        if (!t.streams.empty()) {
            std::vector<uint32_t> rs;
            std::vector<uint64_t> rb, rl, off(1, 0);
            for (int q = 0; q < 40; q++) {
                const uint32_t si = (uint32_t)(rng() % t.streams.size());
                const fl_idx_stream& s = t.streams[si];
                uint64_t on_point = 0;  // a point of the stream, or a byte either side of it
                if (s.n_points) on_point = t.points[s.point0 + rng() % s.n_points].out_pos + rng() % 3 - 1;
                const uint64_t begins[] = {0, s.size, s.size + 1, s.size ? s.size - 1 : 0, ~0ull, ~0ull - rng() % 5, 1ull << 63, rng() % (s.size + 2), on_point};
                const uint64_t begin = begins[rng() % 9];
                const uint64_t lens[] = {0, 1, ~0ull, ~0ull - rng() % 5, 1ull << 63, rng() % (s.size + 2), on_point - begin, on_point - begin + 1};
                const uint64_t len = lens[rng() % 8];
                const uint64_t cap = rng() % 3 == 0 ? rng() % (s.size + 2) : fl_idx_clip(begin, len, s.size) + rng() % 3;
                rs.push_back(si);
                rb.push_back(begin);
                rl.push_back(len);
                off.push_back(off.back() + cap);
            }
            const uint64_t budgets[] = {1, 100, 4096, 1u << 20, ~0ull};
            if (check_call(t, rs, rb, rl, off, budgets[rng() % 5])) return 1;
            fl_idxp_call c;
            fl_idxp_plan_call(t, (uint32_t)rs.size(), rs.data(), rb.data(), rl.data(), off.data(), 1u << 20, c);
            parts_seen += c.parts.size();
        }
        std::free(good);
    }
    CHECK(accepted > 100 && refused > 1000 && parts_seen > 1000);
    std::printf("index_parts_plan ok: %llu mutants accepted, %llu refused, %llu parts cut\n", (unsigned long long)accepted,
                (unsigned long long)refused, (unsigned long long)parts_seen);
    return 0;
}
