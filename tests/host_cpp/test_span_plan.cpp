// The span inflater's host-side decisions (flate_amd/csrc/span_plan.h) over random record sets, hostile ones among them: an
// end_bit anywhere, lengths up to 2^64 - 1, any status.  Built with -fsanitize=address,undefined by
// tests/test_span_plan_cpu.py; needs no GPU.  It checks that every call returns and that every index it hands out lies inside
// its array -- not what the calls decide (tests/test_span_plan_cpu.py does).
#include <cstdio>
#include <cstdlib>

#include "../../flate_amd/csrc/span_plan.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545f4914f6cdd1dull;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("line %d: %s (set %d)\n", __LINE__, #c, set_no); \
            return 1;                                               \
        }                                                           \
    } while (0)

int main() {
    uint32_t xpow8[32];
    xpow8[0] = 0x00800000u;
    for (int j = 1; j < 32; j++) xpow8[j] = fl_crc_mulmod(xpow8[j - 1], xpow8[j - 1]);
    const uint32_t pow_item = fl_crc_xpow8n(xpow8, FP_FIX_ITEM);
    uint64_t closed = 0, items_seen = 0, verified = 0;
    for (int set_no = 0; set_no < 6000; set_no++) {
        const bool hostile = set_no % 3 == 0;
        const uint32_t n_el = 1 + (uint32_t)below(4);
        const bool both = below(2) != 0;
        std::vector<fl_chunk> chunks(n_el, fl_chunk{});
        std::vector<uint32_t> elig(n_el), sp_first(1, 0);
        std::vector<fl_span> spans;
        for (uint32_t k = 0; k < n_el; k++) {
            elig[k] = k;
            chunks[k].in_len = (uint32_t)below(1u << 20);
            chunks[k].in_off = below(1u << 30);
            chunks[k].out_off = below(1ull << 40);
            chunks[k].out_cap = below(4) ? below(1u << 22) : 1u << 22;  // (what bounds the items: a stream never gets more than its room)
            const uint32_t n = 1 + (uint32_t)below(12);
            uint64_t at = 0;
            for (uint32_t j = 0; j < n; j++) {
                fl_span s;
                s.start_bit = at;
                s.wp = rnd();
                s.stream = k;
                s.first = j == 0;
                s.prev = (uint32_t)rnd();
                s.live = (uint32_t)below(2);
                spans.push_back(s);
                at += 1 + below(5000);
            }
            sp_first.push_back((uint32_t)spans.size());
        }
        const uint32_t nsp = (uint32_t)spans.size();
        std::vector<fl_span_res> r1(nsp), r2(nsp);
        for (uint32_t k = 0; k < n_el; k++)
            for (uint32_t j = sp_first[k]; j < sp_first[k + 1]; j++) {
                fl_span_res& r = r1[j];
                const bool last = j + 1 == sp_first[k + 1];
                // mostly a chain that closes: each span ends where the next one starts
                r.end_bit = last ? spans[j].start_bit + 1 + below(5000) : spans[j + 1].start_bit;
                r.out_len = below(3) ? below(3 * FP_FIX_ITEM) : below(2) ? FP_FIX_ITEM * below(4) : 0;
                r.status = 0;
                r.final_seen = last;
                r.uses_hist = (uint32_t)below(2);
                r.n_pieces = (uint32_t)rnd();
                if (below(6) == 0) r.end_bit = spans[sp_first[k] + below(sp_first[k + 1] - sp_first[k])].start_bit;  // any span, itself and earlier ones too
                if (hostile) {
                    switch (below(8)) {
                        case 0: r.end_bit = rnd(); break;
                        case 1: r.end_bit = ~0ull; break;
                        case 2: r.end_bit = spans[j].start_bit; break;
                        case 3: r.out_len = rnd(); break;
                        case 4: r.out_len = ~0ull - below(70000); break;
                        case 5: r.status = (uint32_t)rnd(); break;
                        case 6: r.final_seen = (uint32_t)rnd(); break;
                        default: break;
                    }
                }
                r2[j] = r;
                if (below(10) == 0) r2[j].out_len = rnd();
                if (below(10) == 0) r2[j].status = (uint32_t)below(3);
            }
        // ---- the chains
        std::vector<fl_span_chain> plans(n_el);
        for (uint32_t k = 0; k < n_el; k++) {
            const uint32_t a = sp_first[k], b = sp_first[k + 1];
            const fl_span_chain& pl = plans[k] = fl_span_follow_chain(spans.data(), r1.data(), a, b, chunks[k].out_cap, both);
            CHECK(pl.last >= a && pl.last < b);
            CHECK(pl.chain.size() <= b - a);
            for (size_t q = 0; q < pl.chain.size(); q++) {
                CHECK(pl.chain[q] >= a && pl.chain[q] < b);
                CHECK(q == 0 ? pl.chain[q] == a : pl.chain[q] > pl.chain[q - 1]);
            }
            if (pl.ok) {
                CHECK(pl.total <= chunks[k].out_cap);
                closed++;
            } else {
                for (uint32_t j = a; j < b; j++) CHECK(spans[j].live == 0);
            }
        }
        // ---- the items
        const fl_span_fix_plan fp = fl_span_fix_items(chunks.data(), elig, spans.data(), r1.data(), plans, nsp, both);
        CHECK(fp.items.size() % FP_FIX_WAVES == 0);
        CHECK(fp.item_first.size() == n_el + 1 && fp.chain_off.size() == n_el + 1);
        CHECK(fp.chain_all.size() == fp.chain_pos.size() && fp.chain_all.size() <= nsp && fp.longest <= nsp);
        CHECK(fp.item_first[n_el] == fp.items.size() && fp.chain_off[n_el] == fp.chain_all.size());
        for (uint32_t k = 0; k < n_el; k++) {
            CHECK(fp.item_first[k] <= fp.item_first[k + 1] && fp.chain_off[k] <= fp.chain_off[k + 1]);
            uint64_t bytes = 0;
            for (uint32_t q = fp.item_first[k]; q < fp.item_first[k + 1]; q++) {
                const fl_fix_item& it = fp.items[q];
                CHECK(it.span >= sp_first[k] && it.span < sp_first[k + 1]);
                CHECK(it.len <= FP_FIX_ITEM && it.local % FP_FIX_ITEM == 0 && it.kind <= 3);
                CHECK((uint64_t)it.local + it.len <= r1[it.span].out_len);
                CHECK(it.dst >= chunks[k].out_off && it.dst + it.len <= chunks[k].out_off + chunks[k].out_cap);
                CHECK(it.prev == FP_NO_SPAN ? spans[it.span].first != 0 : it.prev >= sp_first[k] && it.prev < it.span);
                bytes += it.len;
            }
            CHECK(bytes == (plans[k].ok ? plans[k].total : 0));
            items_seen += fp.item_first[k + 1] - fp.item_first[k];
        }
        // ---- the parts and the footers: whatever the device says
        std::vector<uint32_t> part(2 * fp.items.size());
        for (uint32_t& w : part) w = below(4) ? (uint32_t)rnd() : (uint32_t)below(2) * FP_FIX_ITEM;
        std::vector<uint8_t> foot(8 * (size_t)n_el);
        for (uint8_t& f : foot) f = (uint8_t)rnd();
        for (uint32_t k = 0; k < n_el; k++) {
            if (hostile && below(4) == 0) plans[k].end_bit = rnd();
            const int container = (int)below(3);
            const uint32_t flen = fl_span_footer_len(container);
            const uint64_t at = fl_span_footer_at(plans[k], flen, chunks[k].in_len);
            CHECK(at == ~0ull || at + flen <= chunks[k].in_len);
            if (!plans[k].ok) continue;
            const fl_span_verdict v = fl_span_verify(plans[k], spans.data(), r1.data(), below(2) ? r1.data() : r2.data(), below(2) != 0,
                                                     part.data() + 2 * (size_t)fp.item_first[k], fp.item_first[k + 1] - fp.item_first[k],
                                                     container, xpow8, pow_item, &foot[8 * (size_t)k], chunks[k].in_len);
            CHECK(v.bad_b == ~0u || (v.bad_b < plans[k].chain.size() && !v.ok));
            CHECK(!v.ok || v.used <= chunks[k].in_len);
            verified++;
        }
    }
    printf("ok: %llu chains closed, %llu items, %llu streams verified\n", (unsigned long long)closed, (unsigned long long)items_seen,
           (unsigned long long)verified);
    return closed > 1000 && items_seen > 1000 ? 0 : 2;
}
