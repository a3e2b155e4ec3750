// deflater_plan.h -- host side of a resumable huffman-only / store-only feed (flate_hip_deflater_*): which blocks
// a stream's buffered bytes plus its new piece turn into, and what stays buffered.  Plain C++ (no HIP):
// flate_hip.hip uses it, and tests/cpu_shim compiles it for the CPU tests.
#pragma once
#include <stdint.h>

#include <vector>

#include "flate_layout.h"

// device bytes per stream that hold the SimpleCompressor's buffer between feeds (it never holds 65535)
#define FL_DFL_BUF 65536u

enum { FL_FEED_MORE = 0, FL_FEED_FLUSH = 1, FL_FEED_FINISH = 2 };

// The SimpleCompressor (deflate.zig:449-529) writes its 65535-byte buffer out as a block each time it is full;
// flush() writes what it holds (an empty block if nothing) and an empty stored block, finish() writes it as the final
// block.  `bl` buffered bytes followed by `n` new ones: appends the blocks (staged-input-relative byte ranges,
// fl_sblock flags) to `out` and returns how many bytes at the end stay buffered.  Fed the whole stream at once this is
// the block list of flate_hip_compress_batch (in_len / 65535 + 1 blocks) and, with flushes, of
// flate_hip_compress_flush; cut anywhere, the concatenated lists cover the same bytes with the same blocks.
inline uint32_t fl_dfl_blocks(uint32_t bl, uint32_t n, int op, std::vector<fl_sblock>& out) {
    const uint32_t L = bl + n;
    uint32_t p = 0;
    for (; L - p >= FL_BLOCK_BYTES; p += FL_BLOCK_BYTES) out.push_back(fl_sblock{p, FL_BLOCK_BYTES, 0u});
    if (op == FL_FEED_MORE) return L - p;
    out.push_back(fl_sblock{p, L - p, op == FL_FEED_FINISH ? 1u : 0u});
    if (op == FL_FEED_FLUSH) out.push_back(fl_sblock{0u, 0u, 2u});
    return 0;
}

// The piece's checksum units (k_checksum folds at most 65535 bytes per unit): [bl, bl + n) cut at 65535 bytes
inline uint32_t fl_dfl_checksum_units(uint32_t bl, uint32_t n, std::vector<fl_sblock>& out) {
    uint32_t k = 0;
    for (uint32_t p = 0; p < n; p += FL_BLOCK_BYTES, k++) {
        const uint32_t len = n - p < FL_BLOCK_BYTES ? n - p : FL_BLOCK_BYTES;
        out.push_back(fl_sblock{bl + p, len, 0u});
    }
    return k;
}

// Output bytes a feed of `bl + n` bytes can produce at most: the blocks (stored-block bound: 5 bytes per 65535 and
// two more blocks), the container header and footer, the carried byte.
inline uint64_t fl_dfl_out_bound(uint32_t bl, uint32_t n) {
    const uint64_t L = (uint64_t)bl + n;
    return L + 5 * (L / FL_BLOCK_BYTES + 3) + 10 + 8 + 1 + 16;
}
