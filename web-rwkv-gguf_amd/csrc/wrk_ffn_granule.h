// The decode engine's granules of the ffn vector (K5 -> K6): four f16 with the tag in their sign bits.  Free of HIP: the kernel
// (v7_engine_kernel: eng_publish_ffn, eng_sweep_half) and the host test share it.  DESIGN.md section 4.8.  wrk_v7_engine.h includes it.
//
// Every other vector travels as {two f16, 32-bit tag}.  The ffn vector is relu(k)^2 (act_apply(WRK_ACT_SQUARED_RELU): p = fmaxf(x, 0);
// p * p): never negative, never NaN, and -0 * -0 = +0, so bit 15 of each of its f16 is 0 and is free to carry a tag.  A granule is 64
// bits = rows 4 j .. 4 j + 3 in element order (element e in bits [16 e, 16 e + 16)), and bit 15 of element e holds bit e of the 4-bit
// tag (layer % 15) + 1.  The producer MASKS the signs, it does not assume them; the proof above makes the mask a no-op, so the payload
// that unpack returns is bit for bit what the pair form carried.  Half the bytes through the fabric per pass, half the publishing stores.
// Why 4 bits are enough.  A granule location is written once per layer, so a consumer of layer l can meet only the launch's zero, the
// value of layer l - 1, or the value of layer l: a producer writes layer l + 1's ffn vector only after its gather has seen layer l's K6
// output of EVERY workgroup, and a workgroup publishes that output behind the barrier behind which all its waves have read layer l's
// ffn vector.  The tag is never 0 (a zeroed granule never matches) and differs between consecutive layers, also across the wrap
// (layer 14 -> 15, 15 -> 1): nothing older than l - 1 can be met, so the wrap is harmless for any number of layers.
#pragma once
#include <stdint.h>

#ifndef WRK_HD
#ifdef __HIPCC__
#define WRK_HD __host__ __device__
#else
#define WRK_HD
#endif
#endif

namespace wrk {

constexpr uint64_t ENG_FFN_SIGNS = 0x8000800080008000ull;
WRK_HD constexpr uint32_t eng_ffn_nibble(uint32_t layer) { return layer % 15u + 1u; }
// the sign bits of one 32-bit half of a granule (two f16) that carry tag bits b0 (low f16) and b1 (high f16) of `two` (a 2-bit value)
WRK_HD constexpr uint32_t eng_ffn_signs32(uint32_t two) { return ((two & 1u) << 15) | ((two & 2u) << 30); }
WRK_HD constexpr uint64_t eng_ffn_signs(uint32_t nibble) {
    return (uint64_t)eng_ffn_signs32(nibble & 3u) | ((uint64_t)eng_ffn_signs32(nibble >> 2) << 32);
}
// pair01: rows 4 j, 4 j + 1 as two f16 (low first), pair23: rows 4 j + 2, 4 j + 3
WRK_HD constexpr uint64_t eng_ffn_pack(uint32_t pair01, uint32_t pair23, uint32_t nibble) {
    return ((((uint64_t)pair23 << 32) | pair01) & ~ENG_FFN_SIGNS) | eng_ffn_signs(nibble);
}
WRK_HD constexpr bool eng_ffn_match(uint64_t granule, uint32_t nibble) { return (granule & ENG_FFN_SIGNS) == eng_ffn_signs(nibble); }
WRK_HD constexpr uint64_t eng_ffn_payload(uint64_t granule) { return granule & ~ENG_FFN_SIGNS; }
// The properties the hand-off rests on, over the nibble function itself: a broken one does not compile.
constexpr bool eng_ffn_tags_ok() {
    for (uint32_t l = 0; l < 256; ++l) {
        const uint32_t n = eng_ffn_nibble(l);
        if (n == 0 || n > 15u) return false;                                            // four bits, and a zeroed granule never matches
        if (eng_ffn_match(0, n)) return false;
        if (l > 0 && eng_ffn_nibble(l - 1) == n) return false;                          // the previous layer's granule never matches
        if (l > 0 && eng_ffn_match(eng_ffn_pack(0x7fff7fffu, 0x7fff7fffu, eng_ffn_nibble(l - 1)), n)) return false;
        const uint64_t g = eng_ffn_pack(0x3c007bffu, 0x00017c00u, n);                   // 65504, 1.0, +inf, the smallest subnormal
        if (!eng_ffn_match(g, n) || eng_ffn_payload(g) != 0x00017c003c007bffull) return false;
        for (uint32_t e = 0; e < 4; ++e)                                                // a single flipped sign bit never matches
            if (eng_ffn_match(g ^ (0x8000ull << (16u * e)), n)) return false;
        if (eng_ffn_pack(0xbc00fbffu, 0x8001fc00u, n) != g) return false;               // the producer masks: signs in the payload do not leak
    }
    return true;
}
static_assert(eng_ffn_tags_ok(), "ffn granule: a tag that a zeroed or a previous layer's granule can match, or a payload bit lost");

}  // namespace wrk
