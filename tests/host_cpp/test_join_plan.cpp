// join_plan.h under AddressSanitizer and UBSan, as a program of its own (tests/test_join_plan_host_cpp.py builds and
// runs it): random and hostile batches -- empty streams, streams of exactly k pieces and one byte off, pieces of one
// byte, offsets beyond 2^32, streams of more pieces than a call may have -- through the stream table, the piece tables,
// the slots and the bound.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../flate_amd/csrc/join_plan.h"

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                  \
        }                                                              \
    } while (0)

int main() {
    std::mt19937_64 rng(23);
    for (uint32_t r = 0; r < 64; r++) CHECK(fl_join_marker_bytes(r) == (((r & 7) == 0 || (r & 7) >= 6) ? 5u : 4u));
    CHECK(!fl_join_args_ok(65536, 0, 6) && !fl_join_args_ok(1, 3, 6) && !fl_join_args_ok(1, -1, 6) && !fl_join_args_ok(1, 0, 0) &&
          !fl_join_args_ok(1, 0, 1) && !fl_join_args_ok(1, 0, 10) && fl_join_args_ok(0, 2, 9) && fl_join_args_ok(65535, 0, 4));
    for (int it = 0; it < 3000; it++) {
        const uint32_t n = (uint32_t)(rng() % 30);
        const uint32_t piece = fl_join_piece_bytes(rng() % 4 == 0 ? 0u : rng() % 3 == 0 ? (uint32_t)(1 + rng() % 9) : (uint32_t)(1 + rng() % 65535));
        CHECK(piece >= 1 && piece <= FL_JOIN_MAX_PIECE);
        const int container = (int)(rng() % 3);
        std::vector<uint64_t> hin(n + 1), hout(n + 1);
        const uint64_t in_base = rng() % 3 == 0 ? (1ull << 32) + rng() % 1000 : rng() % 100, out_base = rng() % 50;
        uint64_t ia = in_base, oa = out_base, want_pieces = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t k = rng() % 6;
            uint64_t len;
            switch (rng() % 6) {
                case 0: len = 0; break;
                case 1: len = k * piece; break;
                case 2: len = k * piece + 1; break;
                case 3: len = k * piece > 0 ? k * piece - 1 : 0; break;
                default: len = rng() % (4ull * piece + 2); break;
            }
            if (piece < 10 && len > 2000) len %= 2000;
            hin[i] = ia;
            hout[i] = oa;
            ia += len;
            oa += rng() % 8 == 0 ? rng() % 4 : fl_join_bound(len, piece, container);
            want_pieces += len == 0 ? 1 : (len + piece - 1) / piece;
        }
        hin[n] = ia;
        hout[n] = oa;
        const bool host = rng() % 2;
        std::vector<fl_join_stream> s;
        const uint64_t total = fl_join_layout(hin.data(), hout.data(), n, piece, host ? in_base : 0, host ? out_base : 0, s);
        CHECK(total == want_pieces && s.size() == n && total <= FL_JOIN_MAX_PIECES);
        std::vector<uint32_t> ps;
        std::vector<uint64_t> pin, pslot;
        const uint64_t scratch = fl_join_tables(s, piece, total, ps, pin, pslot);
        CHECK(ps.size() == total && pin.size() == total + 1 && pslot.size() == total + 1 && pslot[total] == scratch && pslot[0] == 0);
        uint64_t j = 0;
        for (uint32_t i = 0; i < n; i++) {
            CHECK(s[i].piece0 == j && s[i].n == hin[i + 1] - hin[i] && s[i].out_cap == hout[i + 1] - hout[i]);
            CHECK(s[i].in_off == hin[i] - (host ? in_base : 0) && s[i].out_off == hout[i] - (host ? out_base : 0));
            uint64_t covered = 0, bound = fl_join_hdr_bytes(container) + fl_join_ftr_bytes(container);
            for (uint64_t k = 0; k < s[i].n_pieces; k++, j++) {
                const fl_join_piece p = fl_join_piece_of(s[i], k, piece);
                CHECK(ps[j] == i && pin[j] == p.in_off && pin[j + 1] - pin[j] == p.in_len);
                CHECK(p.in_off == s[i].in_off + covered && p.in_len <= piece && (p.in_len == piece || p.last) && (p.in_len > 0 || s[i].n == 0));
                CHECK(p.last == (k + 1 == s[i].n_pieces ? 1u : 0u));
                const uint64_t slot = pslot[j + 1] - pslot[j];
                CHECK(pslot[j] % FL_JOIN_SLOT_ALIGN == 0 && slot == fl_join_slot_bytes(p.in_len) &&
                      slot >= fl_raw_bound(p.in_len) + FL_JOIN_MARKER_MAX + FL_JOIN_SLOT_SPARE);
                covered += p.in_len;
                bound += fl_raw_bound(p.in_len) + FL_JOIN_MARKER_MAX;
            }
            CHECK(covered == s[i].n && bound == fl_join_bound(s[i].n, piece, container));
        }
        CHECK(j == total);
        if (n) CHECK(pin[total] == s[n - 1].in_off + s[n - 1].n);
    }
    // streams no call can take: counted in closed form, never laid out
    {
        const uint64_t hin[3] = {7, 7 + (1ull << 32) + 5, 7 + (1ull << 33) + 5}, hout[3] = {0, 0, 0};
        std::vector<fl_join_stream> s;
        CHECK(fl_join_layout(hin, hout, 2, 1, 0, 0, s) == (1ull << 33) + 5 - 0 && s[1].piece0 == (1ull << 32) + 5);
        CHECK(fl_join_layout(hin, hout, 2, 1, 0, 0, s) > FL_JOIN_MAX_PIECES);
        CHECK(fl_join_layout(hin, hout, 2, 65535, 0, 0, s) == 65538 + 65538 && s[1].n_pieces == 65538);
        const fl_join_piece p = fl_join_piece_of(s[0], 65537, 65535);
        CHECK(p.last && p.in_off == 7 + 65537ull * 65535 && p.in_len == (1ull << 32) + 5 - 65537ull * 65535);
        CHECK(fl_join_piece_count(~0ull, 1) == ~0ull && fl_join_piece_count(~0ull, 65535) == (~0ull) / 65535);
        CHECK(fl_join_bound((1ull << 32) + 5, 1, 1) == 18 + ((1ull << 32) + 5) * (fl_raw_bound(1) + 5));
    }
    std::printf("join_plan ok\n");
    return 0;
}
