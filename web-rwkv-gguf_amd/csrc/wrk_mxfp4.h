// MXFP4 (WRK_MAT_MXFP4): the stored layout and the launchers of its own kernels (wrk_mxfp4.hip).  The units that route a
// launch by kind include this: wrk_api.hip (create / quantise / export), wrk_matvec.hip and wrk_gemm.hip (the job dispatchers).
//
// Stored row (K % 32 == 0, nblk = K / 32 blocks):
//   code plane   [nblk][16 B]   block b's 32 codes as four dwords; dword d holds elements 8d .. 8d + 7, element 8d + i in bits 4i .. 4i + 3
//                               (ggml keeps element j in the low and element j + 16 in the high nibble of qs[j]: re-ordered on upload)
//   scale plane  [nblk] u8      the E8M0 bytes, block order, right behind the codes
//   padding to 16 bytes: at most 15 bytes per row, none when K % 512 == 0
// so a lane's block is one aligned 16-byte load, a lane's MFMA fragment one dword of it, and 64 lanes fetch 64 consecutive scale bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "wrk_matjob.h"

namespace wrk {

struct MatvecParams;

inline size_t mxfp4_row_bytes(uint32_t k) { return (k & 31u) ? 0 : (((size_t)k / 2 + k / 32 + 15) & ~(size_t)15); }

// one row of ggml blocks { u8 e; u8 qs[16] } -> one stored row (dst zero-filled by the caller)
inline void mxfp4_row_to_stored(uint32_t k, const uint8_t* src, uint8_t* dst) {
    for (uint32_t b = 0; b < k / 32; ++b) {
        const uint8_t* blk = src + (size_t)b * 17;
        uint8_t* code = dst + (size_t)b * 16;
        for (uint32_t i = 0; i < 32; ++i) {
            const uint8_t c = (blk[1 + (i & 15u)] >> (i < 16 ? 0 : 4)) & 15u;
            code[i >> 1] |= (uint8_t)(c << (4 * (i & 1u)));
        }
        dst[k / 2 + b] = blk[0];
    }
}

// the inverse: one stored row -> ggml blocks, bit for bit
inline void mxfp4_row_from_stored(uint32_t k, const uint8_t* src, uint8_t* dst) {
    for (uint32_t b = 0; b < k / 32; ++b) {
        const uint8_t* code = src + (size_t)b * 16;
        uint8_t* blk = dst + (size_t)b * 17;
        blk[0] = src[k / 2 + b];
        memset(blk + 1, 0, 16);
        for (uint32_t i = 0; i < 32; ++i) {
            const uint8_t c = (code[i >> 1] >> (4 * (i & 1u))) & 15u;
            blk[1 + (i & 15u)] |= (uint8_t)(c << (i < 16 ? 0 : 4));
        }
    }
}

// f16 [m][k] -> stored rows by the OCP MX rule (include/wrk_hip.h, wrk_matrix_quantize); dst zero-filled by the caller
void quantize_mxfp4(hipStream_t s, const void* src_f16, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes);

// decode matvec: every job of P is MXFP4, workgroups cut as matvec() cuts them (rows_per_wg, wg_begin; total_wg in all).  Any number of
// tokens (1 .. 4 per pass).  0 = launched (or would be, dry), -3 = a job asks for a fused prologue / carry / gate, -1 = no launch
int mxfp4_matvec(hipStream_t s, const MatvecParams& P, uint32_t total_wg, uint32_t ntok, bool dry);

// prefill GEMM on the matrix cores: every job is MXFP4 and multiplies the same tokens.  -2 = a job is not for this path (too few tokens,
// views that are no dense stacks, M % 4): the caller uses the matvec kernels
int mxfp4_gemm(hipStream_t s, const MatJob* jobs, int njobs, uint32_t min_tokens, int num_cu);

}  // namespace wrk
