// CPU build of the span inflater's host-side decisions (flate_amd/csrc/span_plan.h).
// TEST INFRASTRUCTURE ONLY: lets the tuning rules, the walk over a stream's span records, the work items of k_span_fix and
// the checksum fold be checked without a GPU.  Not linked into libflate_hip.so.
#include "../../flate_amd/csrc/span_plan.h"

namespace {

std::vector<fl_chunk> chunks_of(const uint32_t* in_len, const uint64_t* out_cap, const uint64_t* out_off, uint32_t n) {
    std::vector<fl_chunk> c(n, fl_chunk{});
    for (uint32_t i = 0; i < n; i++) {
        c[i].in_len = in_len[i];
        c[i].out_cap = out_cap ? out_cap[i] : 0;
        c[i].out_off = out_off ? out_off[i] : 0;
    }
    return c;
}

// records as six words each: end_bit, out_len, status, final_seen, uses_hist, n_pieces
std::vector<fl_span_res> records_of(const uint64_t* rec6, uint32_t n) {
    std::vector<fl_span_res> r(n);
    for (uint32_t i = 0; i < n; i++) {
        r[i].end_bit = rec6[6 * i];
        r[i].out_len = rec6[6 * i + 1];
        r[i].status = (uint32_t)rec6[6 * i + 2];
        r[i].final_seen = (uint32_t)rec6[6 * i + 3];
        r[i].uses_hist = (uint32_t)rec6[6 * i + 4];
        r[i].n_pieces = (uint32_t)rec6[6 * i + 5];
    }
    return r;
}

// spans as five words each: start_bit, wp, first, prev, live (in and out)
std::vector<fl_span> spans_of(const uint64_t* sp5, uint32_t n) {
    std::vector<fl_span> s(n);
    for (uint32_t i = 0; i < n; i++) {
        s[i].start_bit = sp5[5 * i];
        s[i].wp = sp5[5 * i + 1];
        s[i].stream = 0;
        s[i].first = (uint32_t)sp5[5 * i + 2];
        s[i].prev = (uint32_t)sp5[5 * i + 3];
        s[i].live = (uint32_t)sp5[5 * i + 4];
    }
    return s;
}
void spans_back(const std::vector<fl_span>& s, uint64_t* sp5) {
    for (size_t i = 0; i < s.size(); i++) {
        sp5[5 * i] = s[i].start_bit;
        sp5[5 * i + 1] = s[i].wp;
        sp5[5 * i + 2] = s[i].first;
        sp5[5 * i + 3] = s[i].prev;
        sp5[5 * i + 4] = s[i].live;
    }
}

}  // namespace

extern "C" {

// 0 FP_TAIL, 1 FP_NO_SPAN, 2 FP_FIX_ITEM, 3 FP_FIX_WAVES, 4 FL_SPAN_STREAMS, 5 FL_SPAN_BYTES, 6 FL_SPAN_MAX, 7 FP_PIECE
uint32_t shim_span_const(int which) {
    const uint32_t v[] = {FP_TAIL, FP_NO_SPAN, FP_FIX_ITEM, FP_FIX_WAVES, FL_SPAN_STREAMS, FL_SPAN_BYTES, FL_SPAN_MAX, FP_PIECE};
    return v[which];
}

// the streams that are cut: writes their indices and *twin, returns the count
int shim_span_eligible(const uint32_t* in_len, uint32_t n, uint64_t min_bytes, int flags, uint32_t n_cu, int twin_knob, uint32_t* out,
                       int* twin) {
    const std::vector<fl_chunk> c = chunks_of(in_len, nullptr, nullptr, n);
    const fl_span_elig e = fl_span_eligible(c.data(), n, min_bytes, flags, n_cu, twin_knob);
    for (size_t i = 0; i < e.elig.size(); i++) out[i] = e.elig[i];
    *twin = e.twin ? 1 : 0;
    return (int)e.elig.size();
}

// the scan targets of the eligible streams: (from_bit, limit_bit, stream) triples and pt_first[n_elig + 1]; returns the
// count of targets (only `cap` of them are written)
int shim_span_targets(const uint32_t* in_len, const uint64_t* out_cap, uint32_t n, const uint32_t* elig, uint32_t n_elig, int twin,
                      int twin_knob, int sym, uint32_t n_cu, uint64_t* out3, int cap, uint32_t* pt_first) {
    const std::vector<fl_chunk> c = chunks_of(in_len, out_cap, nullptr, n);
    std::vector<fl_scan_point> pts;
    std::vector<uint32_t> first;
    fl_span_targets(c.data(), std::vector<uint32_t>(elig, elig + n_elig), twin != 0, twin_knob, sym != 0, n_cu, pts, first);
    for (int i = 0; i < (int)pts.size() && i < cap; i++) {
        out3[3 * i] = pts[i].from_bit;
        out3[3 * i + 1] = pts[i].limit_bit;
        out3[3 * i + 2] = pts[i].stream;
    }
    for (size_t k = 0; k < first.size(); k++) pt_first[k] = first[k];
    return (int)pts.size();
}

int shim_cut_positions(const uint64_t* found, uint32_t j0, uint32_t j1, uint64_t limit_bit, uint64_t* out) {
    const std::vector<uint64_t> p = fl_cut_positions(found, j0, j1, limit_bit);
    for (size_t i = 0; i < p.size(); i++) out[i] = p[i];
    return (int)p.size();
}

// the spans of a batch: (start_bit, stream, first, prev, live, wp) per span, cand, cand_off[n_chunks + 1],
// sp_first[n_elig + 1]; returns the count of spans (room for one per stream and one per target is the caller's)
int shim_span_build(uint32_t n_chunks, const uint32_t* elig, uint32_t n_elig, const uint32_t* pt_first, const uint64_t* found,
                    uint64_t* out6, uint64_t* cand, uint32_t* cand_off, uint32_t* sp_first) {
    std::vector<fl_span> spans;
    std::vector<uint64_t> cd;
    std::vector<uint32_t> co, sf;
    fl_span_build(n_chunks, std::vector<uint32_t>(elig, elig + n_elig), std::vector<uint32_t>(pt_first, pt_first + n_elig + 1), found, spans, cd,
                  co, sf);
    for (size_t i = 0; i < spans.size(); i++) {
        const uint64_t w[6] = {spans[i].start_bit, spans[i].stream, spans[i].first, spans[i].prev, spans[i].live, spans[i].wp};
        for (int q = 0; q < 6; q++) out6[6 * i + q] = w[q];
    }
    for (size_t i = 0; i < cd.size(); i++) cand[i] = cd[i];
    for (size_t i = 0; i < co.size(); i++) cand_off[i] = co[i];
    for (size_t i = 0; i < sf.size(); i++) sp_first[i] = sf[i];
    return (int)spans.size();
}

uint64_t shim_span_pool_pieces(const uint32_t* in_len, const uint64_t* out_cap, uint32_t n, const uint32_t* elig, uint32_t n_elig,
                               uint32_t nsp, int both) {
    const std::vector<fl_chunk> c = chunks_of(in_len, out_cap, nullptr, n);
    return fl_span_pool_pieces(c.data(), std::vector<uint32_t>(elig, elig + n_elig), nsp, both != 0);
}

// the chain of the stream whose spans are [a, b) of sp5 / rec6 (n entries each).  Writes the spans back, the chain, and
// res4 = (total, end_bit, last, chain length); returns ok
int shim_span_follow_chain(uint64_t* sp5, const uint64_t* rec6, uint32_t n, uint32_t a, uint32_t b, uint64_t out_cap, int both,
                           uint32_t* chain, uint64_t* res4) {
    std::vector<fl_span> s = spans_of(sp5, n);
    const std::vector<fl_span_res> r = records_of(rec6, n);
    const fl_span_chain pl = fl_span_follow_chain(s.data(), r.data(), a, b, out_cap, both != 0);
    spans_back(s, sp5);
    for (size_t i = 0; i < pl.chain.size(); i++) chain[i] = pl.chain[i];
    res4[0] = pl.total;
    res4[1] = pl.end_bit;
    res4[2] = pl.last;
    res4[3] = pl.chain.size();
    return pl.ok ? 1 : 0;
}

// The work items of a batch of n_elig streams (stream k: out_off[k], spans [sp_first[k], sp_first[k + 1]) of sp5 / rec6).
// The chains are followed here, with out_cap[k]; ok[k] says which closed.  Items as seven words each: dst, span, local,
// len, kind, prev, pad (room for `cap` of them).  misc3 = (count of items, longest, uses_hist); chain_all / chain_pos have
// room for nsp entries, chain_off and item_first for n_elig + 1.
void shim_span_fix_items(const uint64_t* out_off, const uint64_t* out_cap, uint32_t n_elig, const uint32_t* sp_first, uint64_t* sp5,
                         const uint64_t* rec6, int both, int32_t* ok, uint64_t* items7, uint32_t cap, uint32_t* item_first,
                         uint32_t* chain_all, uint32_t* chain_off, uint32_t* chain_pos, uint64_t* misc3) {
    const uint32_t nsp = sp_first[n_elig];
    std::vector<fl_span> s = spans_of(sp5, nsp);
    const std::vector<fl_span_res> r = records_of(rec6, nsp);
    std::vector<fl_chunk> c(n_elig, fl_chunk{});
    std::vector<uint32_t> elig(n_elig);
    std::vector<fl_span_chain> plans(n_elig);
    for (uint32_t k = 0; k < n_elig; k++) {
        c[k].out_off = out_off[k];
        c[k].out_cap = out_cap[k];
        elig[k] = k;
        plans[k] = fl_span_follow_chain(s.data(), r.data(), sp_first[k], sp_first[k + 1], out_cap[k], both != 0);
        ok[k] = plans[k].ok ? 1 : 0;
    }
    spans_back(s, sp5);
    const fl_span_fix_plan fp = fl_span_fix_items(c.data(), elig, s.data(), r.data(), plans, nsp, both != 0);
    for (size_t i = 0; i < fp.items.size() && i < cap; i++) {
        const fl_fix_item& it = fp.items[i];
        const uint64_t w[7] = {it.dst, it.span, it.local, it.len, it.kind, it.prev, it.pad};
        for (int q = 0; q < 7; q++) items7[7 * i + q] = w[q];
    }
    for (size_t i = 0; i < fp.item_first.size(); i++) item_first[i] = fp.item_first[i];
    for (size_t i = 0; i < fp.chain_all.size(); i++) chain_all[i] = fp.chain_all[i];
    for (size_t i = 0; i < fp.chain_pos.size(); i++) chain_pos[i] = fp.chain_pos[i];
    for (size_t i = 0; i < fp.chain_off.size(); i++) chain_off[i] = fp.chain_off[i];
    misc3[0] = fp.items.size();
    misc3[1] = fp.longest;
    misc3[2] = fp.uses_hist ? 1 : 0;
}

// One closed chain (spans chain[0 .. n_chain) of first[] / rec6_a / rec6_b, nsp entries each) against its items' parts
// and its footer.  res3 = (used, crc, bad_b); returns ok
int shim_span_verify(const uint32_t* chain, uint32_t n_chain, uint64_t total, uint64_t end_bit, const uint32_t* first, const uint64_t* rec6_a,
                     const uint64_t* rec6_b, uint32_t nsp, int uses_hist, const uint32_t* part, uint32_t n_parts, int container,
                     const uint8_t* foot, uint64_t in_len, uint64_t* res3) {
    uint32_t xpow8[32];
    xpow8[0] = 0x00800000u;  // x^8 in the reflected representation (x^0 = 0x80000000)
    for (int j = 1; j < 32; j++) xpow8[j] = fl_crc_mulmod(xpow8[j - 1], xpow8[j - 1]);
    std::vector<fl_span> s(nsp, fl_span{});
    for (uint32_t i = 0; i < nsp; i++) s[i].first = first[i];
    const std::vector<fl_span_res> ra = records_of(rec6_a, nsp), rb = records_of(rec6_b, nsp);
    fl_span_chain pl;
    pl.ok = true;
    pl.chain.assign(chain, chain + n_chain);
    pl.total = total;
    pl.end_bit = end_bit;
    const fl_span_verdict v = fl_span_verify(pl, s.data(), ra.data(), rb.data(), uses_hist != 0, part, n_parts, container, xpow8,
                                             fl_crc_xpow8n(xpow8, FP_FIX_ITEM), foot, in_len);
    res3[0] = v.used;
    res3[1] = v.crc;
    res3[2] = v.bad_b;
    return v.ok ? 1 : 0;
}

}  // extern "C"
