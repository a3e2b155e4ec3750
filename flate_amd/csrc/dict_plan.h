// dict_plan.h -- host side of inflate with preset dictionaries (flate_hip_decompress_batch_dict,
// flate_hip_inflater_set_dictionary): the checks of the call's arguments and the table of dictionaries the kernels read.
// Plain C++ (no HIP types): flate_hip.hip uses it, kernels_inflate.h shares the table's record, and tests/cpu_shim
// compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#include <vector>

#define FL_DICT_WINDOW 32768u     // bytes of a dictionary that a match can reach: its tail
#define FL_DICT_NONE 0xffffffffu  // in dict_of: this stream has no dictionary

// one dictionary of a call
struct fl_dict_ent {
    uint64_t start, end;  // dict[start, end): all of it, which the Adler-32 of a zlib stream's DICTID covers
    uint32_t hist_len;    // min(end - start, FL_DICT_WINDOW): dict[end - hist_len, end) is the history of its streams
    uint32_t adler;       // filled on the device (k_dict_adler)
};

// What the call may be given.  container: 0 (raw) and 2 (zlib) carry dictionaries, gzip has no such thing.  dict_off:
// n_dicts + 1 ascending offsets (host copy).  dict_of: one entry per stream, a dictionary's index or FL_DICT_NONE; null
// only when there is exactly one dictionary, which every stream then uses.  False: FLATE_HIP_E_INVALID_ARG.
inline bool fl_dict_args_ok(int container, const uint64_t* dict_off, uint32_t n_dicts, const uint32_t* dict_of,
                            bool have_dict_of, uint32_t n_chunks) {
    if (container != 0 && container != 2) return false;
    if (n_dicts == FL_DICT_NONE) return false;
    if (n_dicts && !dict_off) return false;
    for (uint32_t d = 0; d < n_dicts; d++)
        if (dict_off[d + 1] < dict_off[d]) return false;
    if (!have_dict_of) return n_dicts == 1;
    if (!dict_of) return n_chunks == 0;
    for (uint32_t i = 0; i < n_chunks; i++)
        if (dict_of[i] != FL_DICT_NONE && dict_of[i] >= n_dicts) return false;
    return true;
}

// The table of the call's dictionaries (adler is left 0: the device fills it).
inline void fl_dict_table(const uint64_t* dict_off, uint32_t n_dicts, std::vector<fl_dict_ent>& tab) {
    tab.resize(n_dicts);
    for (uint32_t d = 0; d < n_dicts; d++) {
        const uint64_t len = dict_off[d + 1] - dict_off[d];
        tab[d].start = dict_off[d];
        tab[d].end = dict_off[d + 1];
        tab[d].hist_len = len < FL_DICT_WINDOW ? (uint32_t)len : FL_DICT_WINDOW;
        tab[d].adler = 0;
    }
}
