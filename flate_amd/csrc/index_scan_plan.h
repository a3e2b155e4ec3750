// index_scan_plan.h -- host side of flate_hip_index_scan: a fresh seek index (index_parts_plan.h) over streams somebody
// else wrote, found by walking the stream -- nothing is decoded into memory.  Which block starts are candidates, which
// of them are kept, which of the kept ones are fresh, and how the records the device walkers (kernels_index_scan.h)
// hand over become the points.  Plain C++ (no HIP types): flate_hip.hip uses it, tests/cpu_shim and tests/host_cpp
// compile it for the CPU tests.
//
// A MARK of a stream is a block start whose preceding block is a stored block with LEN 0 and BFINAL 0: the trailer of a
// sync or full flush.  It lies on a byte boundary by construction.
//
// KEPT MARKS.  pos[0] = 0 is block 0, behind it the positions of the marks in stream order; fl_idx_point_rule over that
// sequence with fl_idx_spacing(spacing) says which are kept -- the rule fl_idxp_point_pieces applies to piece starts.
//
// FRESHNESS.  A kept mark at output position c is fresh iff no match token at a position p >= c has p - distance < c
// (only p < c + 32768 can matter): a decoder that starts there needs no window.
//
// POINTS.  Block 0 and the fresh kept marks; in_bit and out_pos ascend strictly.  A kept mark that is not fresh is
// dropped, not replaced: where it is a sync flush, the full flush further on in its cell is not looked for.  A stream
// without fresh marks has point 0 alone.
//
// What the device hands over, per walk (a whole stream, or a live span of the size probe's chain): a list of entries
// (in_bit, out_pos, need), need being the largest distance - (p - out_pos) over the matches between this entry and the
// next, or 0.  Entry 0 of every list carries the walk's start and is no mark; the others are marks the walk kept by the
// cell comparison among its own marks.  A walk inside a stream does not know the last mark in front of it: it lists its
// first mark whatever its cell, and its record tells the position of its last mark, kept or not, so that the rule can be
// applied here to every walk's first mark against the last mark of the walks before it.  A listed mark that this drops
// only constrains, as the walk starts do.
#pragma once
#include <stdint.h>

#include <vector>

#include "index_plan.h"

struct fl_ixs_entry {
    uint64_t in_bit;   // the BFINAL bit of the block that starts here, from the stream's first byte
    uint64_t out_pos;  // bytes produced before it
    uint64_t need;     // how far the matches between this entry and the next reach in front of out_pos, at most
};
#define FL_IXS_MARKER_BITS 32u       // a marker takes more bits than this: three of header, the padding, LEN and NLEN
#define FL_IXS_COPY_WHOLE 4096u      // with room for at most this many entries the lists come home as they are, unpacked

// entries a walk of out_len bytes lists, at most: its start, its first mark, and a mark per grid line in (base, base +
// out_len] ...
inline uint64_t fl_ixs_max_entries(uint64_t out_len, uint64_t spacing) { return 3 + out_len / spacing; }
// ... of which a walk over in_bits bits of input holds fewer than in_bits / FL_IXS_MARKER_BITS: every mark has a marker
// of its own in front of it, inside the walk.  max_points: fl_idx_max_points of the walk, 1 + out_len / spacing.
inline uint64_t fl_ixs_walk_entries(uint64_t max_points, uint64_t in_bits) {
    const uint64_t by_bits = 1 + in_bits / FL_IXS_MARKER_BITS;
    return 2 + (max_points < by_bits ? max_points : by_bits);
}

// one walk as the host sees it: its list and what its record says
struct fl_ixs_walk {
    const fl_ixs_entry* e;
    uint64_t n;          // entries, e[0] (the start) included
    uint64_t out_len;    // bytes the walk's blocks produce
    uint64_t last_mark;  // has_mark: the position of the walk's last mark, kept or not
    uint32_t has_mark;
    uint32_t first;      // the walk starts at the stream's first block: it applied the rule to its first mark itself
};

// The points of one stream of `size` bytes from its walks in stream order.  false: the lists contradict the probe that
// said the stream is good and `size` bytes long, or themselves -- no walk, a list without its start, a start that is
// not where the walks before it ended, lengths that do not add up to size, positions that descend or leave the walk, a
// match that reaches in front of the stream's first byte (a first entry with need > 0 is one), a listed mark that
// cannot have been kept, a last mark in front of a listed one.  Nothing of the input is believed: sums are checked
// before they are made.
inline bool fl_ixs_points(const fl_ixs_walk* w, uint64_t n_walks, uint64_t size, uint64_t spacing, std::vector<fl_idx_point>& out) {
    const uint64_t sp = fl_idx_spacing(spacing);
    const size_t out0 = out.size();  // (a refusal leaves `out` as it was)
    if (!n_walks || !w[0].first) return false;
    // ---- the lists are consistent; which listed marks are kept
    std::vector<const fl_ixs_entry*> ent;
    std::vector<uint8_t> kept;
    uint64_t base = 0, prev_mark = 0;  // bytes in front of walk k; the last mark in front of it (block 0: position 0)
    for (uint64_t k = 0; k < n_walks; k++) {
        const fl_ixs_walk& a = w[k];
        if (a.n < 1 || !a.e || a.out_len > size - base || (k > 0 && a.first)) return false;
        const uint64_t end = base + a.out_len;
        if (a.e[0].out_pos != base) return false;
        for (uint64_t q = 0; q < a.n; q++) {
            const fl_ixs_entry& e = a.e[q];
            if (e.out_pos < base || e.out_pos > end || e.need > e.out_pos) return false;
            bool is = false;
            if (q >= 1) {
                const fl_ixs_entry& p = a.e[q - 1];
                if (e.out_pos < p.out_pos || e.in_bit <= p.in_bit) return false;
                // the walk compared with the mark in front (q >= 2, or the first walk), which lies at or behind p
                if (q >= 2 || a.first) {
                    if (!(e.out_pos / sp > p.out_pos / sp)) return false;
                    is = true;
                } else {
                    is = e.out_pos / sp > prev_mark / sp;
                }
            } else if (!ent.empty() && e.in_bit < ent.back()->in_bit) {
                return false;
            }
            ent.push_back(&e);
            kept.push_back(is ? 1 : 0);
        }
        if (a.has_mark) {
            if (a.last_mark < a.e[a.n - 1].out_pos || a.last_mark > end) return false;
            prev_mark = a.last_mark;
        } else if (a.n > 1) {
            return false;
        }
        base = end;
    }
    if (base != size) return false;
    // ---- freshness: one backward running minimum of out_pos - need
    std::vector<uint8_t> fresh(ent.size(), 0);
    uint64_t low = ~0ull;
    for (size_t k = ent.size(); k-- > 0;) {
        const uint64_t reach = ent[k]->out_pos - ent[k]->need;  // (need <= out_pos: checked above)
        if (reach < low) low = reach;
        fresh[k] = kept[k] && low >= ent[k]->out_pos;
    }
    out.push_back(fl_idx_point{ent[0]->in_bit, 0, 0});
    uint64_t last_bit = ent[0]->in_bit, last_pos = 0;
    for (size_t k = 1; k < ent.size(); k++) {
        if (!fresh[k]) continue;
        if (ent[k]->out_pos <= last_pos || ent[k]->in_bit <= last_bit) {  // (kept marks ascend strictly by their cells)
            out.resize(out0);
            return false;
        }
        out.push_back(fl_idx_point{ent[k]->in_bit, ent[k]->out_pos, 0});
        last_bit = ent[k]->in_bit;
        last_pos = ent[k]->out_pos;
    }
    return true;
}
