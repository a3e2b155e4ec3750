// CPU shim over flate_amd/csrc/dict_plan.h for tests/test_dict_cases_cpu.py: the argument checks and the table of
// dictionaries of flate_hip_decompress_batch_dict, as plain C functions.
#include "../../flate_amd/csrc/dict_plan.h"

extern "C" {

uint32_t shim_dict_const(int i) {
    switch (i) {
        case 0: return FL_DICT_WINDOW;
        case 1: return FL_DICT_NONE;
        case 2: return (uint32_t)sizeof(fl_dict_ent);
        default: return 0;
    }
}

// have_dict_of = 0: the caller passed NULL for dict_of
int shim_dict_args_ok(int container, const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of, int have_dict_of,
                      uint32_t n_chunks) {
    return fl_dict_args_ok(container, dict_off, n_dicts, dict_of, have_dict_of != 0, n_chunks) ? 1 : 0;
}

// start / end / hist_len / adler of every dictionary
void shim_dict_table(const uint64_t* dict_off, uint32_t n_dicts, uint64_t* start, uint64_t* end, uint32_t* hist_len,
                     uint32_t* adler) {
    std::vector<fl_dict_ent> tab;
    fl_dict_table(dict_off, n_dicts, tab);
    for (uint32_t d = 0; d < n_dicts; d++) {
        start[d] = tab[d].start;
        end[d] = tab[d].end;
        hist_len[d] = tab[d].hist_len;
        adler[d] = tab[d].adler;
    }
}
}
