// CPU shim over flate_amd/csrc/index_scan_plan.h for tests/test_index_scan_plan_cpu.py: the host decision of
// flate_hip_index_scan -- the walkers' lists of one stream to its points -- as a plain C function.
#include "../../flate_amd/csrc/index_scan_plan.h"

extern "C" {

uint64_t shim_ixs_max_entries(uint64_t out_len, uint64_t spacing) { return fl_ixs_max_entries(out_len, spacing); }
uint64_t shim_ixs_copy_whole(void) { return FL_IXS_COPY_WHOLE; }
uint64_t shim_ixs_walk_entries(uint64_t max_points, uint64_t in_bits) { return fl_ixs_walk_entries(max_points, in_bits); }

// Walk k has n_entries[k] rows of in_bit | out_pos | need in `entries`, one walk's behind the other's.  Returns -1 when
// the lists are refused, else the number of points; pts (in_bit | out_pos rows) is filled as far as room allows.
int64_t shim_ixs_points(uint64_t n_walks, const uint64_t* n_entries, const uint64_t* out_len, const uint64_t* last_mark,
                        const uint32_t* has_mark, const uint32_t* first, const uint64_t* entries, uint64_t size, uint64_t spacing,
                        uint64_t* pts, uint64_t room) {
    std::vector<fl_ixs_entry> e;
    std::vector<fl_ixs_walk> w;
    uint64_t total = 0;
    for (uint64_t k = 0; k < n_walks; k++) total += n_entries[k];
    for (uint64_t q = 0; q < total; q++) e.push_back(fl_ixs_entry{entries[3 * q], entries[3 * q + 1], entries[3 * q + 2]});
    uint64_t at = 0;
    for (uint64_t k = 0; k < n_walks; k++) {
        w.push_back(fl_ixs_walk{e.data() + at, n_entries[k], out_len[k], last_mark[k], has_mark[k], first[k]});
        at += n_entries[k];
    }
    std::vector<fl_idx_point> p;
    if (!fl_ixs_points(w.data(), w.size(), size, spacing, p)) return p.empty() ? -1 : -2;  // (a refusal leaves nothing behind)
    for (size_t k = 0; k < p.size() && k < room; k++) {
        pts[2 * k] = p[k].in_bit;
        pts[2 * k + 1] = p[k].out_pos;
    }
    return (int64_t)p.size();
}
}
