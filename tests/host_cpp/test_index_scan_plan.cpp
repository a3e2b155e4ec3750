// flate_amd/csrc/index_scan_plan.h under AddressSanitizer and UBSan (tests/test_index_scan_host_cpp.py builds and runs it):
// random and hostile lists of the walkers of flate_hip_index_scan -- positions, lengths and needs near 2^64, lists
// without their start, walks that overlap or leave gaps, marks out of order -- through fl_ixs_points, every list in a heap
// array of exactly its size.  Every input is refused with nothing left behind, or accepted with everything true that the
// version-2 blob's validator and the part decoder rely on: point 0 at output byte 0, in_bit and out_pos ascending
// strictly, out_pos within size, at most 1 + size / spacing points -- and with exactly the points of a quadratic
// restatement of the rule.
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <random>

#include "../../flate_amd/csrc/index_scan_plan.h"

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            fails++;                                              \
        }                                                         \
    } while (0)

struct Lists {
    std::vector<std::unique_ptr<fl_ixs_entry[]>> mem;  // (exactly n entries each: a read past the end is ASan's)
    std::vector<fl_ixs_walk> w;
    void add(const std::vector<fl_ixs_entry>& e, uint64_t out_len, uint64_t last_mark, uint32_t has_mark, uint32_t first) {
        mem.emplace_back(new fl_ixs_entry[e.size()]);
        for (size_t k = 0; k < e.size(); k++) mem.back()[k] = e[k];
        w.push_back(fl_ixs_walk{mem.back().get(), e.size(), out_len, last_mark, has_mark, first});
    }
};

// the definition, quadratic: valid lists only
static std::vector<fl_idx_point> by_definition(const Lists& L, uint64_t spacing) {
    std::vector<fl_ixs_entry> all;
    std::vector<int> kept;
    uint64_t prev = 0;
    for (const fl_ixs_walk& a : L.w) {
        for (uint64_t q = 0; q < a.n; q++) {
            all.push_back(a.e[q]);
            kept.push_back(q == 0 ? 0 : (q >= 2 || a.first) ? 1 : a.e[q].out_pos / spacing > prev / spacing);
        }
        if (a.has_mark) prev = a.last_mark;
    }
    std::vector<fl_idx_point> out;
    out.push_back(fl_idx_point{all[0].in_bit, 0, 0});
    for (size_t k = 1; k < all.size(); k++) {
        bool fresh = kept[k] != 0;
        for (size_t j = k; j < all.size() && fresh; j++) fresh = all[j].need <= all[j].out_pos - all[k].out_pos;
        if (fresh) out.push_back(fl_idx_point{all[k].in_bit, all[k].out_pos, 0});
    }
    return out;
}

static void check_accepted(const std::vector<fl_idx_point>& p, size_t p0, uint64_t size, uint64_t spacing) {
    const uint64_t sp = fl_idx_spacing(spacing);
    CHECK(p.size() > p0);
    if (p.size() <= p0) return;
    CHECK(p[p0].out_pos == 0);
    CHECK(p.size() - p0 - 1 <= size / sp);
    for (size_t k = p0; k < p.size(); k++) {
        CHECK(p[k].out_pos <= size && p[k].win_off == 0);
        if (k > p0) CHECK(p[k].out_pos > p[k - 1].out_pos && p[k].in_bit > p[k - 1].in_bit);
    }
}

// valid lists of a stream that begins at output byte 0 and whose positions are lifted by `lift` behind the first walk's
// start (lift near 2^64: the sums of the decision may not wrap)
static void random_valid(std::mt19937_64& g, uint64_t lift) {
    const uint64_t spc[] = {1, 2, 7, 100, 4096, 1ull << 20};
    const uint64_t spacing = spc[g() % 6];
    Lists L;
    const int n_walks = 1 + (int)(g() % 5);
    uint64_t pos = 0, bit = g() % 200, prev_mark = 0;
    for (int w = 0; w < n_walks; w++) {
        std::vector<fl_ixs_entry> e;
        const uint64_t base = pos;
        e.push_back(fl_ixs_entry{bit, pos, 0});
        uint64_t last_mark = 0, in_walk_prev = prev_mark;
        uint32_t has_mark = 0;
        const int n_marks = (int)(g() % 6);
        for (int m = 0; m < n_marks; m++) {
            const uint64_t step = (g() % 3 == 0 ? 0 : g() % (3 * spacing + 2)) + (w == 0 && m == 0 ? lift : 0);
            pos += step;
            bit += 8 + g() % 4000;
            const bool listed = (w > 0 && !has_mark) || pos / spacing > in_walk_prev / spacing;
            in_walk_prev = pos;
            last_mark = pos;
            has_mark = 1;
            if (listed) e.push_back(fl_ixs_entry{bit, pos, 0});
        }
        pos += g() % (2 * spacing + 3);
        bit += 3 + g() % 100;
        for (fl_ixs_entry& x : e) {  // needs: none, exactly to an earlier listed position, one byte further, anything
            const uint64_t far = x.out_pos < 32768 ? x.out_pos : 32768;
            switch (g() % 4) {
                case 0: x.need = 0; break;
                case 1: x.need = far ? g() % (far + 1) : 0; break;
                case 2: x.need = x.out_pos - base <= far ? x.out_pos - base : 0; break;
                default: x.need = x.out_pos - base + 1 <= far ? x.out_pos - base + 1 : 0; break;
            }
        }
        if (w == 0) e[0].need = 0;
        L.add(e, pos - base, last_mark, has_mark, w == 0);
        if (has_mark) prev_mark = last_mark;
    }
    std::vector<fl_idx_point> got(3, fl_idx_point{1, 2, 3});  // (the points are appended)
    const bool ok = fl_ixs_points(L.w.data(), L.w.size(), pos, spacing, got);
    CHECK(ok);
    if (!ok) return;
    check_accepted(got, 3, pos, spacing);
    const std::vector<fl_idx_point> want = by_definition(L, spacing);
    CHECK(got.size() - 3 == want.size());
    for (size_t k = 0; k < want.size() && k + 3 < got.size(); k++) CHECK(got[k + 3].in_bit == want[k].in_bit && got[k + 3].out_pos == want[k].out_pos);
}

static uint64_t hostile_value(std::mt19937_64& g) {
    switch (g() % 6) {
        case 0: return ~0ull - g() % 4;
        case 1: return (1ull << 63) + g() % 3 - 1;
        case 2: return g() % 5;
        case 3: return g();
        case 4: return 32768 + g() % 3 - 1;
        default: return g() % 100000;
    }
}

static void random_hostile(std::mt19937_64& g) {
    Lists L;
    const int n_walks = (int)(g() % 4);
    for (int w = 0; w < n_walks; w++) {
        std::vector<fl_ixs_entry> e;
        const int n = (int)(g() % 5);
        for (int k = 0; k < n; k++) e.push_back(fl_ixs_entry{hostile_value(g), hostile_value(g), hostile_value(g)});
        L.add(e, hostile_value(g), hostile_value(g), (uint32_t)(g() % 2), g() % 4 ? (uint32_t)(w == 0) : (uint32_t)(g() % 2));
    }
    const uint64_t size = hostile_value(g), spacing = g() % 3 ? hostile_value(g) : 0;
    std::vector<fl_idx_point> got(2, fl_idx_point{9, 9, 9});
    if (fl_ixs_points(L.w.data(), L.w.size(), size, spacing, got))
        check_accepted(got, 2, size, spacing);
    else
        CHECK(got.size() == 2);
}

// a valid pair of walks with one field made hostile
static void mutated(std::mt19937_64& g) {
    Lists L;
    L.add({{80, 0, 0}, {800, 100, 0}, {2400, 300, 1}}, 500, 300, 1, 1);
    L.add({{4000, 500, 0}, {4800, 600, 0}, {7200, 900, 0}}, 500, 900, 1, 0);
    fl_ixs_walk& a = L.w[g() % 2];
    fl_ixs_entry& e = L.mem[g() % 2][g() % 3];
    uint64_t size = 1000;
    switch (g() % 8) {
        case 0: e.in_bit = hostile_value(g); break;
        case 1: e.out_pos = hostile_value(g); break;
        case 2: e.need = hostile_value(g); break;
        case 3: a.out_len = hostile_value(g); break;
        case 4: a.last_mark = hostile_value(g); break;
        case 5: a.n = g() % 4; break;
        case 6: size = hostile_value(g); break;
        default: a.has_mark = 0; break;
    }
    std::vector<fl_idx_point> got;
    const uint64_t spacing = g() % 2 ? 1 : 100;
    if (fl_ixs_points(L.w.data(), L.w.size(), size, spacing, got))
        check_accepted(got, 0, size, spacing);
    else
        CHECK(got.empty());
}

int main() {
    std::mt19937_64 g(20240611);
    for (int i = 0; i < 4000; i++) random_valid(g, 0);
    for (int i = 0; i < 2000; i++) random_valid(g, ~0ull - (1ull << 40) - g() % 1000);
    for (int i = 0; i < 20000; i++) random_hostile(g);
    for (int i = 0; i < 20000; i++) mutated(g);
    // the two contradictions the walkers' records can hold
    {
        Lists L;
        L.add({{80, 0, 1}}, 10, 0, 0, 1);
        std::vector<fl_idx_point> got;
        CHECK(!fl_ixs_points(L.w.data(), 1, 10, 1, got) && got.empty());
        Lists M;
        M.add({{80, 0, 0}}, 10, 0, 0, 1);
        CHECK(!fl_ixs_points(M.w.data(), 1, 11, 1, got) && got.empty());
        CHECK(fl_ixs_points(M.w.data(), 1, 10, 1, got) && got.size() == 1);
    }
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok\n");
    return 0;
}
