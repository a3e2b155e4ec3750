// index_plan.h under AddressSanitizer and UBSan, as a program of its own (tests/test_index_plan_host_cpp.py builds and
// runs it): a few thousand truncated, bit-flipped and field-mutated blobs through the validator -- each is refused, or
// accepted with every invariant the decoder relies on true -- and hostile range lists (begins near 2^64, begin + len
// past it) through clipping, point selection, the scratch slots and the passes.  Every blob lies in a heap array of
// exactly its size, so one byte read beyond it is seen.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../flate_amd/csrc/index_plan.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

// a table as the build leaves it: random streams, a part of them failed, points by the rule over random block sizes
static void random_tab(std::mt19937_64& rng, fl_idx_tab& t) {
    t = fl_idx_tab();
    t.container = (uint32_t)(rng() % 3);
    const uint64_t spacings[] = {1, 3, 1000, 32768, 1u << 20};
    t.spacing = spacings[rng() % 5];
    const uint32_t ns = (uint32_t)(rng() % 6);
    for (uint32_t i = 0; i < ns; i++) {
        fl_idx_stream s{};
        s.point0 = t.points.size();
        if (rng() % 4 == 0) {
            s.in_len = rng() % 100;
            s.status = 1 + (int32_t)(rng() % 14);
        } else {
            std::vector<uint64_t> pos(1, 0), which;
            const uint32_t nb = (uint32_t)(1 + rng() % 12);
            for (uint32_t k = 1; k < nb; k++) pos.push_back(pos.back() + (rng() % 3 == 0 ? 0 : rng() % (3 * t.spacing + 2)));
            s.size = pos.back() + rng() % 50;
            fl_idx_point_rule(pos.data(), pos.size(), t.spacing, which);
            s.n_points = which.size();
            s.in_len = 2 + 3 * nb + rng() % 1000;
            for (uint64_t k : which) {
                t.points.push_back(fl_idx_point{3 + 20 * k + rng() % 8, pos[k], t.win_bytes});
                t.win_bytes += fl_idx_window_len(pos[k]);
            }
        }
        t.streams.push_back(s);
    }
}

// what fl_idx_blob_parse promises of a blob it accepts
static bool invariants(const fl_idx_tab& t, uint64_t bytes, uint64_t win_at) {
    if (t.container > 2 || t.spacing == 0) return false;
    if (win_at > bytes || bytes - win_at != t.win_bytes) return false;
    if (win_at != FL_IDX_HDR_BYTES + (uint64_t)FL_IDX_STREAM_BYTES * t.streams.size() + (uint64_t)FL_IDX_POINT_BYTES * t.points.size()) return false;
    uint64_t at = 0, win = 0;
    for (const fl_idx_stream& s : t.streams) {
        if (s.point0 != at || s.n_points > t.points.size() - at) return false;
        if (s.status != 0 && (s.n_points || s.size)) return false;
        if (s.status == 0 && (s.n_points < 1 || s.n_points - 1 > s.size / t.spacing)) return false;  // (1 + size / spacing may be 2^64)
        for (uint64_t k = 0; k < s.n_points; k++) {
            const fl_idx_point& p = t.points[at + k];
            if (p.win_off != win || p.in_bit >= s.in_len * 8 || p.out_pos > s.size) return false;
            if (k == 0 ? p.out_pos != 0 : (p.out_pos <= t.points[at + k - 1].out_pos || p.in_bit <= t.points[at + k - 1].in_bit)) return false;
            win += fl_idx_window_len(p.out_pos);
            if (win > t.win_bytes) return false;
        }
        at += s.n_points;
    }
    return at == t.points.size() && win == t.win_bytes;
}

int main() {
    std::mt19937_64 rng(41);
    uint64_t accepted = 0, refused = 0;
    for (int it = 0; it < 400; it++) {
        fl_idx_tab t;
        random_tab(rng, t);
        const uint64_t n = fl_idx_blob_bytes(t);
        uint8_t* good = (uint8_t*)std::malloc(n);
        CHECK(good);
        const uint64_t at = fl_idx_blob_write(t, good);
        CHECK(at + t.win_bytes == n);
        for (uint64_t b = at; b < n; b++) good[b] = (uint8_t)rng();
        fl_idx_tab back;
        uint64_t win_at = 0;
        CHECK(fl_idx_blob_parse(good, n, back, &win_at) && win_at == at && invariants(back, n, win_at));
        CHECK(back.streams.size() == t.streams.size() && back.points.size() == t.points.size() && back.win_bytes == t.win_bytes);
        for (size_t k = 0; k < t.points.size(); k++)
            CHECK(back.points[k].in_bit == t.points[k].in_bit && back.points[k].out_pos == t.points[k].out_pos &&
                  back.points[k].win_off == t.points[k].win_off);
        // ---- mutants: each in an array of exactly its size
        for (int m = 0; m < 12; m++) {
            uint64_t len = n;
            const int kind = (int)(rng() % 4);
            if (kind == 0) len = rng() % (n + 1);                       // truncated
            if (kind == 1 && rng() % 2) len = n + 1 + rng() % 40;       // something behind it
            uint8_t* mut = (uint8_t*)std::malloc(len ? len : 1);
            CHECK(mut);
            for (uint64_t b = 0; b < len; b++) mut[b] = b < n ? good[b] : (uint8_t)rng();
            const uint64_t tables = at < len ? at : len;
            if (kind == 2 && tables) {  // bits of the tables flipped
                for (int f = 0, nf = 1 + (int)(rng() % 3); f < nf; f++) mut[rng() % tables] ^= (uint8_t)(1u << (rng() % 8));
            }
            if (kind == 3 && tables >= 8) {  // a field replaced: a small number, a huge one, one near a power of two
                const uint64_t field = (rng() % (tables / 8)) * 8;
                const uint64_t vals[] = {0, 1, rng() % 100, ~0ull, ~0ull - rng() % 100, 1ull << 32, (1ull << 63) + rng() % 3, rng()};
                fl_idx_put64(mut + field, vals[rng() % 8]);
            }
            fl_idx_tab got;
            uint64_t wa = 0;
            if (fl_idx_blob_parse(len ? mut : nullptr, len, got, &wa)) {
                CHECK(invariants(got, len, wa));
                accepted++;
            } else {
                refused++;
            }
            std::free(mut);
        }
        // ---- hostile ranges against the good table
        for (int q = 0; q < 40 && !t.streams.empty(); q++) {
            const uint32_t si = (uint32_t)(rng() % t.streams.size());
            const fl_idx_stream& s = t.streams[si];
            const uint64_t begins[] = {0, s.size, s.size + 1, s.size ? s.size - 1 : 0, ~0ull, ~0ull - rng() % 5, 1ull << 63, rng() % (s.size + 2)};
            const uint64_t lens[] = {0, 1, ~0ull, ~0ull - rng() % 5, 1ull << 63, rng() % (s.size + 2)};
            const uint64_t begin = begins[rng() % 8], len = lens[rng() % 6], cap = rng() % 3 == 0 ? rng() % (s.size + 2) : ~0ull;
            const uint64_t lp = fl_idx_clip(begin, len, s.size);
            CHECK(lp <= len && (begin >= s.size ? lp == 0 : lp <= s.size - begin));
            const fl_idx_range r = fl_idx_plan_range(t, si, begin, len, cap);
            if (s.status != 0) {
                CHECK(!r.decode && r.status == s.status && r.len == 0);
            } else if (lp > cap) {
                CHECK(!r.decode && r.status == 100 && r.len == 0);
            } else if (lp == 0) {
                CHECK(!r.decode && r.status == 0 && r.len == 0);
            } else {
                CHECK(r.decode && r.status == 0 && r.len == lp && r.point >= s.point0 && r.point < s.point0 + s.n_points);
                const fl_idx_point& p = t.points[r.point];
                CHECK(p.out_pos <= begin && r.skip == begin - p.out_pos);
                CHECK(r.point + 1 == s.point0 + s.n_points || t.points[r.point + 1].out_pos > begin);
                CHECK(r.skip + r.len <= s.size);
                CHECK(r.in_lo == p.in_bit >> 3 && r.in_lo < r.in_hi && r.in_hi <= s.in_len);
                for (uint64_t k = r.point + 1; k < s.point0 + s.n_points; k++)  // behind the first point at or behind the range's end
                    if (t.points[k].out_pos >= begin + r.len) {
                        CHECK(r.in_hi > t.points[k].in_bit >> 3);
                        break;
                    }
                const uint64_t slot = fl_idx_slot_bytes(r.skip + r.len);
                CHECK(slot % FL_IDX_SLOT_ALIGN == 0 && slot >= r.skip + r.len + FL_IDX_SLACK);
            }
        }
        std::free(good);
    }
    CHECK(accepted > 100 && refused > 1000);
    // ---- the passes: slots near 2^64 must not wrap the sum
    {
        std::vector<uint64_t> first, off;
        const uint64_t slots[] = {~0ull - 15, 16, 0, ~0ull - 31, 32, 32};
        fl_idx_passes(slots, 6, 64, first, off);
        CHECK(first.size() == 5 && first[1] == 1 && first[2] == 3 && first[3] == 4 && first[4] == 6);
        CHECK(off[0] == 0 && off[1] == 0 && off[2] == 16 && off[3] == 0 && off[4] == 0 && off[5] == 32);
    }
    std::printf("index_plan ok: %llu mutants accepted, %llu refused\n", (unsigned long long)accepted, (unsigned long long)refused);
    return 0;
}
