// dict_plan.h under AddressSanitizer and UBSan, as a program of its own (tests/test_dict_cases_cpu.py builds and runs it):
// the argument checks and the table of dictionaries over random and hostile offset tables.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../flate_amd/csrc/dict_plan.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    std::mt19937_64 rng(5);
    for (int it = 0; it < 20000; it++) {
        const uint32_t n_dicts = (uint32_t)(rng() % 6), n_chunks = (uint32_t)(rng() % 9);
        // exactly n_dicts + 1 offsets and n_chunks entries on the heap: a read past either is caught
        std::vector<uint64_t> off(n_dicts + 1);
        uint64_t at = rng() % 100;
        bool ascending = true;
        for (uint32_t d = 0; d <= n_dicts; d++) {
            off[d] = at;
            const uint64_t step = rng() % 8 == 0 ? 0 : rng() % 70000;
            if (rng() % 50 == 0 && at > 0) {
                at -= 1 + rng() % at;  // a descending pair
                if (d < n_dicts) ascending = false;
            } else {
                at += step;
            }
        }
        std::vector<uint32_t> of(n_chunks);
        bool in_range = true;
        for (uint32_t i = 0; i < n_chunks; i++) {
            const uint64_t r = rng() % 10;
            of[i] = r == 0 ? FL_DICT_NONE : r == 1 ? (uint32_t)rng() : n_dicts ? (uint32_t)(rng() % n_dicts) : FL_DICT_NONE;
            if (of[i] != FL_DICT_NONE && of[i] >= n_dicts) in_range = false;
        }
        const int container = (int)(rng() % 5) - 1;
        const bool cont_ok = container == 0 || container == 2;
        const bool with_of = rng() % 3 != 0;
        const bool got = fl_dict_args_ok(container, off.data(), n_dicts, with_of ? of.data() : nullptr, with_of, n_chunks);
        const bool want = cont_ok && ascending && (with_of ? in_range : n_dicts == 1);
        CHECK(got == want);
        if (!ascending) continue;
        std::vector<fl_dict_ent> tab;
        fl_dict_table(off.data(), n_dicts, tab);
        CHECK(tab.size() == n_dicts);
        for (uint32_t d = 0; d < n_dicts; d++) {
            const uint64_t len = off[d + 1] - off[d];
            CHECK(tab[d].start == off[d] && tab[d].end == off[d + 1] && tab[d].adler == 0);
            CHECK(tab[d].hist_len == (len < 32768 ? len : 32768));
            CHECK(tab[d].end - tab[d].hist_len >= tab[d].start);  // the tail lies inside the dictionary
        }
    }
    // no dictionaries at all: dict_off may be null
    const uint32_t none[2] = {FL_DICT_NONE, FL_DICT_NONE};
    const uint64_t zero[1] = {0};
    CHECK(fl_dict_args_ok(0, zero, 0, none, true, 2));
    CHECK(!fl_dict_args_ok(0, nullptr, 1, none, true, 2));
    std::puts("dict_plan ok");
    return 0;
}
