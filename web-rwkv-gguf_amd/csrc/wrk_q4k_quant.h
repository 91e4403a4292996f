// The on-device Q4_K quantiser (wrk_q4k_quant.hip): f16 rows -> Q4_K super-blocks by ggml's scale search, written in the
// stored layout of WRK_MAT_Q4_K (repack_rows, wrk_matvec.hip).  wrk_api.hip includes this for wrk_matrix_quantize / wrk_matrix_export.
//
// Stored row (K % 256 == 0, nb = K / 256 super-blocks), as wrk_matrix_create lays out ggml's 144-byte blocks { d, dmin, scales[12], qs[128] }:
//   code plane    [nb][128 B]   qs as in the block: byte l of 64-element group g holds element 64g + l low, element 64g + 32 + l high
//   header plane  [nb][4 B]     d, dmin (f16)
//   scale plane   [nb][16 B]    the sixteen 6-bit values unpacked, group g as [sc(2g), sc(2g + 1), m(2g), m(2g + 1)]
//   padding to 16 bytes
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

namespace wrk {

// one stored row -> ggml's 144-byte blocks, bit for bit (the inverse of repack_rows: the scale plane back into the 6-bit packing)
inline void q4k_row_from_stored(uint32_t k, const uint8_t* src, uint8_t* dst) {
    const size_t nb = k / 256;
    for (size_t b = 0; b < nb; ++b) {
        uint8_t* blk = dst + b * 144;
        const uint8_t* u = src + nb * 132 + b * 16;
        uint8_t sc[8], mn[8];
        for (int j = 0; j < 8; ++j) {
            sc[j] = u[(j >> 1) * 4 + (j & 1)];
            mn[j] = u[(j >> 1) * 4 + 2 + (j & 1)];
        }
        memcpy(blk, src + nb * 128 + b * 4, 4);
        for (int j = 0; j < 4; ++j) {
            blk[4 + j] = (uint8_t)((sc[j] & 63) | ((sc[j + 4] >> 4) << 6));
            blk[8 + j] = (uint8_t)((mn[j] & 63) | ((mn[j + 4] >> 4) << 6));
            blk[12 + j] = (uint8_t)((sc[j + 4] & 15) | ((mn[j + 4] & 15) << 4));
        }
        memcpy(blk + 16, src + b * 128, 128);
    }
}

// f16 [m][k] -> stored rows by the rule of include/wrk_hip.h (wrk_matrix_quantize, WRK_MAT_Q4_K); the caller zero-fills dst's padding
void quantize_q4_k(hipStream_t s, const void* src_f16, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes);

}  // namespace wrk
