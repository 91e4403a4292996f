// Host program of tests/test_engine_ffn_granule_host.py: the decode engine's four-value granules of the ffn vector
// (web-rwkv-gguf_amd/csrc/wrk_ffn_granule.h, included alone: it is free of HIP), exhaustively.  Built under the address and
// undefined-behaviour sanitizers.  What a granule must look like is restated here from the layout as the header's comment gives it
// (element e in bits [16 e, 16 e + 16), bit 15 of element e = bit e of (layer % 15) + 1), never through the header's own functions.
#include <cstdint>
#include <cstdio>

#include "wrk_ffn_granule.h"

using namespace wrk;

static uint64_t want_granule(const uint16_t (&el)[4], uint32_t tag) {
    uint64_t g = 0;
    for (int e = 0; e < 4; ++e) g |= (uint64_t)((el[e] & 0x7fffu) | (((tag >> e) & 1u) << 15)) << (16 * e);
    return g;
}

int main() {
    unsigned long long round_trips = 0, bad_pack = 0, bad_payload = 0, no_match = 0, wrong_match = 0, flip_match = 0, mask_leak = 0;
    // every sign-clear f16 pattern (+0 = 0x0000, +inf = 0x7c00 and the NaN encodings among them) in each position under every tag
    for (uint32_t tag = 1; tag <= 15; ++tag)
        for (int pos = 0; pos < 4; ++pos)
            for (uint32_t p = 0; p < 0x8000u; ++p) {
                uint16_t el[4];
                for (int e = 0; e < 4; ++e) el[e] = (uint16_t)((p * 40503u + 977u * (uint32_t)e + 31u * tag) & 0x7fffu);     // the other three: anything sign-clear
                el[pos] = (uint16_t)p;
                const uint32_t p01 = el[0] | ((uint32_t)el[1] << 16), p23 = el[2] | ((uint32_t)el[3] << 16);
                const uint64_t g = eng_ffn_pack(p01, p23, tag);
                ++round_trips;
                if (g != want_granule(el, tag)) ++bad_pack;
                if (eng_ffn_payload(g) != (((uint64_t)p23 << 32) | p01)) ++bad_payload;
                if (!eng_ffn_match(g, tag)) ++no_match;
                for (uint32_t other = 0; other <= 15; ++other)
                    if (other != tag && eng_ffn_match(g, other)) ++wrong_match;
                for (int e = 0; e < 4; ++e)
                    if (eng_ffn_match(g ^ (0x8000ull << (16 * e)), tag)) ++flip_match;
                // a producer that is handed set sign bits masks them
                if (eng_ffn_pack(p01 | 0x80008000u, p23 | 0x80008000u, tag) != g) ++mask_leak;
            }
    // layers: the tag is (l % 15) + 1; neither the launch's zero nor the previous layer's granule, whatever its payload, matches
    unsigned long long layers = 0, bad_tag = 0, zero_match = 0, prev_match = 0, prev_checked = 0;
    for (uint32_t l = 0; l < 64; ++l) {
        ++layers;
        const uint32_t tag = eng_ffn_nibble(l);
        if (tag != l % 15u + 1u || tag == 0 || tag > 15u) ++bad_tag;
        if (eng_ffn_match(0, tag)) ++zero_match;
        if (l == 0) continue;
        const uint32_t prev = eng_ffn_nibble(l - 1);
        for (uint32_t p = 0; p < 0x8000u; ++p) {
            const uint32_t pp = p | (p << 16);
            ++prev_checked;
            if (eng_ffn_match(eng_ffn_pack(pp, pp, prev), tag)) ++prev_match;
        }
    }
    // a few granules as the header makes them, for the test to set against its own restatement of the layout
    printf("{\"round_trips\": %llu, \"bad_pack\": %llu, \"bad_payload\": %llu, \"no_match\": %llu, \"wrong_match\": %llu, \"flip_match\": %llu, "
           "\"mask_leak\": %llu, \"layers\": %llu, \"bad_tag\": %llu, \"zero_match\": %llu, \"prev_checked\": %llu, \"prev_match\": %llu, \"samples\": [",
           round_trips, bad_pack, bad_payload, no_match, wrong_match, flip_match, mask_leak, layers, bad_tag, zero_match, prev_checked, prev_match);
    const uint16_t sample[4] = {0x3c00, 0x7bff, 0x0001, 0x7c00};     // 1.0, 65504, the smallest subnormal, +inf
    for (uint32_t l = 0; l < 33; ++l)
        printf("%s[%u, \"%016llx\"]", l ? ", " : "", l,
               (unsigned long long)eng_ffn_pack(sample[0] | ((uint32_t)sample[1] << 16), sample[2] | ((uint32_t)sample[3] << 16), eng_ffn_nibble(l)));
    printf("]}\n");
    return 0;
}
