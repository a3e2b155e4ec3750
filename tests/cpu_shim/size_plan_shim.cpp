// CPU build of the size probe's host-side decisions (flate_amd/csrc/size_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the spacing of the scan targets and the rule that follows a stream's chain of span
// records be checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/size_plan.h"

extern "C" {

int shim_size_span_bytes() { return (int)FL_SZ_SPAN_BYTES; }
int shim_size_span_max() { return (int)FL_SZ_SPAN_MAX; }
int shim_size_streams_max() { return (int)FL_SZ_STREAMS_MAX; }

// the streams of a batch that are cut: writes their indices, returns the count
int shim_size_eligible(const uint64_t* in_len, uint32_t n, uint64_t min_bytes, uint32_t n_cu, uint32_t* out) {
    std::vector<uint32_t> e;
    fl_size_eligible(in_len, n, min_bytes, n_cu, e);
    for (uint32_t i = 0; i < (uint32_t)e.size(); i++) out[i] = e[i];
    return (int)e.size();
}

// pieces per eligible stream
void shim_size_spacing(const uint64_t* in_len, uint32_t n, uint32_t n_cu, uint32_t* pieces) {
    std::vector<uint32_t> p;
    fl_size_spacing(in_len, n, n_cu, p);
    for (uint32_t i = 0; i < n; i++) pieces[i] = p[i];
}

// the scan targets of one stream: writes up to `cap` (from, limit) pairs, returns the count of pairs
int shim_size_targets(uint64_t in_len, uint32_t p, uint64_t* out, int cap) {
    std::vector<uint64_t> v;
    fl_size_targets(in_len, p, v);
    for (int i = 0; i < (int)v.size() && i < 2 * cap; i++) out[i] = v[i];
    return (int)(v.size() / 2);
}

// spans as (start_bit, first) and records as (end_bit, out_len, need_hist, consumed, status, final_seen), six words each
int shim_size_follow_chain(const uint64_t* start_bit, const uint64_t* rec6, uint32_t n, uint64_t* size, int32_t* status,
                           uint64_t* consumed) {
    std::vector<fl_size_span> sp(n);
    std::vector<fl_size_rec> rc(n);
    for (uint32_t i = 0; i < n; i++) {
        sp[i].start_bit = start_bit[i];
        sp[i].stop_bit = i + 1 < n ? start_bit[i + 1] : ~0ull;
        sp[i].stream = 0;
        sp[i].first = i == 0;
        rc[i].end_bit = rec6[6 * i];
        rc[i].out_len = rec6[6 * i + 1];
        rc[i].need_hist = rec6[6 * i + 2];
        rc[i].consumed = rec6[6 * i + 3];
        rc[i].status = (int32_t)rec6[6 * i + 4];
        rc[i].final_seen = (uint32_t)rec6[6 * i + 5];
    }
    return fl_size_follow_chain(sp.data(), rc.data(), n, size, status, consumed) ? 1 : 0;
}

}  // extern "C"
