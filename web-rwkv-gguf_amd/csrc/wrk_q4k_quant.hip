// f16 -> Q4_K on gfx950: ggml's quantize_row_q4_K_ref as a kernel.  Per 32-element sub-block the (scale, min) pair comes
// from a search over 22 candidate grids, each fitted by weighted least squares (weights sqrt(mean x^2) + |x|); per 256-element super-block
// the eight pairs are put on two 6-bit grids under the f16 factors d and dmin, and the 4-bit codes are then taken from that stored header.
//
// Work split: one wave per super-block, the 8 lanes 8j .. 8j + 7 own sub-block j, a lane holds elements 4i .. 4i + 3 of it (one 8-byte
// load; a wave reads 512 contiguous bytes, the four waves of a workgroup four consecutive super-blocks) in registers through all
// candidates.  Every sum of a candidate meets inside its 8 lanes by three DPP steps (quad xor 1, quad xor 2, half mirror); each step adds
// the same two values in both lanes of a pair, so the 8 lanes hold the same bits and take the same decisions without a broadcast.  The
// sub-blocks of a wave decide differently, so a candidate is kept by selects, never by a branch.  The header maxima cross the eight
// sub-blocks once (row mirror, then two lane exchanges).  Sub-blocks 2g and 2g + 1 share the bytes of group g: the odd one hands its
// codes to the even one through a rotate by 8 lanes inside the 16-lane row, and the even one stores whole dwords.  No LDS, no barrier.
//
// All arithmetic is f32 with the compiler's correctly rounded division and square root and no contraction (-ffp-contract=off), so the
// final codes are reproducible from the stored header with the same expression on any IEEE machine.
#include "wrk_device.h"
#include "wrk_q4k_quant.h"

namespace wrk {

namespace {

constexpr int Q4K_NSTEP = 20;       // candidates is = 0 .. 20: iscale = (14 + 0.1 is) / (max - min)

// sum / max / min over the 8 lanes of a sub-block, the same bits in every one of them
__device__ __forceinline__ float sub_sum(float v) {
    v += dpp_f32<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);     // row_half_mirror
    return v;
}
__device__ __forceinline__ float sub_max(float v) {
    v = fmaxf(v, dpp_f32<0xB1>(v));
    v = fmaxf(v, dpp_f32<0x4E>(v));
    return fmaxf(v, dpp_f32<0x141>(v));
}
__device__ __forceinline__ float sub_min(float v) {
    v = fminf(v, dpp_f32<0xB1>(v));
    v = fminf(v, dpp_f32<0x4E>(v));
    return fminf(v, dpp_f32<0x141>(v));
}
// max over the eight sub-blocks of a value that is uniform inside each
__device__ __forceinline__ float block_max(float v) {
    v = fmaxf(v, dpp_f32<0x140>(v));        // row_mirror: the other sub-block of the 16-lane row
    v = fmaxf(v, __shfl_xor(v, 16, WAVE));
    return fmaxf(v, __shfl_xor(v, 32, WAVE));
}
// the value of the lane 8 away inside the 16-lane row (row_ror:8)
__device__ __forceinline__ uint32_t partner(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true); }

__device__ __forceinline__ float code_of(float v, float top) { return fminf(fmaxf(rintf(v), 0.0f), top); }     // a NaN becomes 0

// the weighted squared error of the grid (scale, mn) with codes l
__device__ __forceinline__ float grid_error(const float (&x)[4], const float (&w)[4], const float (&l)[4], float scale, float mn) {
    float e = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float diff = scale * l[i] + mn - x[i];
        e += w[i] * (diff * diff);
    }
    return sub_sum(e);
}

}  // namespace

__global__ void __launch_bounds__(256) q4k_quant_kernel(const f16* __restrict__ src, uint8_t* __restrict__ dst, uint32_t nb, uint64_t total,
                                                        uint32_t row_bytes) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t sb = (uint64_t)blockIdx.x * 4 + wave;        // super-block of the flattened [m][nb] matrix
    if (sb >= total) return;                                    // whole waves leave: EXEC stays full for the DPP steps, no barrier below
    const uint32_t j = lane >> 3, i = lane & 7;

    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    const f16x4 raw = *(const f16x4*)(src + sb * 256 + lane * 4);
    const float x[4] = {(float)raw[0], (float)raw[1], (float)raw[2], (float)raw[3]};

    // ---- the sub-block's weights, range and the sums every candidate shares
    const float av = sqrtf(sub_sum((x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3])) / 32.0f);
    float w[4], sw = 0.0f, sx = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        w[e] = av + fabsf(x[e]);
        sw += w[e];
        sx += w[e] * x[e];
    }
    sw = sub_sum(sw);
    sx = sub_sum(sx);
    const float mx = sub_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    const float mn = fminf(sub_min(fminf(fminf(x[0], x[1]), fminf(x[2], x[3]))), 0.0f);
    const bool flat = mx == mn;
    const float range = flat ? 1.0f : mx - mn;

    // ---- the search: start from the min/max grid, keep a fitted candidate only when its error is strictly smaller
    float l[4];
    float scale, minv = mn, best;
    {
        const float iscale = 15.0f / range;
        scale = 1.0f / iscale;
#pragma unroll
        for (int e = 0; e < 4; ++e) l[e] = code_of(iscale * (x[e] - mn), 15.0f);
        best = grid_error(x, w, l, scale, mn);
    }
    for (int is = 0; is <= Q4K_NSTEP; ++is) {
        const float iscale = (-1.0f + 0.1f * (float)is + 15.0f) / range;
        float sl = 0.0f, sl2 = 0.0f, sxl = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            l[e] = code_of(iscale * (x[e] - mn), 15.0f);
            const float wl = w[e] * l[e];
            sl += wl;
            sl2 += wl * l[e];
            sxl += wl * x[e];
        }
        sl = sub_sum(sl);
        sl2 = sub_sum(sl2);
        sxl = sub_sum(sxl);
        const float D = sw * sl2 - sl * sl;
        float ts = (sw * sxl - sx * sl) / D;
        float tm = (sl2 * sx - sl * sxl) / D;
        if (tm > 0.0f) {
            tm = 0.0f;
            ts = sxl / sl2;
        }
        const float err = grid_error(x, w, l, ts, tm);
        const bool take = D > 0.0f && err < best;       // a NaN error never wins
        best = take ? err : best;
        scale = take ? ts : scale;
        minv = take ? tm : minv;
    }
    if (flat) { scale = 0.0f; minv = mn; }
    const float off = 0.0f - minv;                      // the stored offset, >= 0 (and +0, never -0)

    // ---- the super-block's header: both maxima, the 6-bit codes under them
    const float max_scale = block_max(scale), max_off = block_max(off);
    const float inv_scale = max_scale > 0.0f ? 63.0f / max_scale : 0.0f;
    const float inv_off = max_off > 0.0f ? 63.0f / max_off : 0.0f;
    const float ls = code_of(inv_scale * scale, 63.0f), lm = code_of(inv_off * off, 63.0f);
    const f16 d16 = (f16)(max_scale / 63.0f), dmin16 = (f16)(max_off / 63.0f);

    // ---- the codes, from the header as it is stored
    const float d = (float)d16 * ls, dm = (float)dmin16 * lm;
    uint32_t codes = 0;
    if (d != 0.0f) {
#pragma unroll
        for (int e = 0; e < 4; ++e) codes |= (uint32_t)code_of((x[e] + dm) / d, 15.0f) << (8 * e);
    }

    // ---- stores: sub-block 2g gives the low, 2g + 1 the high nibbles of group g's bytes 4i .. 4i + 3
    const uint32_t row = (uint32_t)(sb / nb), b = (uint32_t)(sb % nb);
    uint8_t* out = dst + (size_t)row * row_bytes;
    const uint32_t pair = (uint32_t)ls | ((uint32_t)lm << 16);
    const uint32_t codes_hi = partner(codes), pair_hi = partner(pair);
    if ((j & 1u) == 0) {
        *(uint32_t*)(out + (size_t)b * 128 + (j >> 1) * 32 + i * 4) = codes | (codes_hi << 4);
        if (i == 0) *(uint32_t*)(out + (size_t)nb * 132 + (size_t)b * 16 + (j >> 1) * 4) = pair | (pair_hi << 8);
    }
    if (lane == 0)
        *(uint32_t*)(out + (size_t)nb * 128 + (size_t)b * 4) =
            (uint32_t)__builtin_bit_cast(uint16_t, d16) | ((uint32_t)__builtin_bit_cast(uint16_t, dmin16) << 16);
}

void quantize_q4_k(hipStream_t s, const void* src_f16, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes) {
    const uint32_t nb = k / 256;
    const uint64_t total = (uint64_t)nb * m;
    hipLaunchKernelGGL(q4k_quant_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, s, (const f16*)src_f16, dst, nb, total, row_bytes);
}

}  // namespace wrk
