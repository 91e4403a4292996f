// Row arithmetic shared by the kernels that work on rows of f32 logits [rows][V] (wrk_sample.hip, wrk_score.hip, wrk_logprob.hip,
// wrk_penalty.hip): the sampler's order, the (max, sum) pair of a log-sum-exp with its one merge and its one finish, the steps
// of a pass over a row in register tiles, and the gate that says whether a row's draw counts.  Each exists once, here, so that two files
// that promise the same bits or the same order run the same expression.  See DESIGN.md §7.
#pragma once
#include "wrk_device.h"

namespace wrk {

// ------------------------------------------------------------------ the sampler's order
// a logit as every order reads it: NaN counts as -inf (p = 0); -0 becomes +0 (ties go by index, not by sign bit)
__device__ __forceinline__ float row_norm(float l) { return l != l ? -INFINITY : l + 0.0f; }

// tokens by logit descending, ties by index ascending, as one 52-bit key monotone(logit) << 20 | (2^20 - 1 - index) of a row_norm'ed
// logit: unique per token and never 0
__device__ __forceinline__ uint64_t rank_key(float l, uint32_t i) {
    uint32_t b = __float_as_uint(l);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)b << 20) | (0xFFFFFu - i);
}

// ------------------------------------------------------------------ log-sum-exp as a (max, sum) pair
// (m, s) <- the pair for the union of the two sets.  m is never NaN (fmaxf drops NaN operands); a NaN logit makes s NaN, which every later
// merge keeps.  s == 0 with m == -inf is the empty set.
__device__ __forceinline__ void row_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float a = s == 0.0f ? 0.0f : (m == mn ? s : s * expf(m - mn));
    const float b = s2 == 0.0f ? 0.0f : (m2 == mn ? s2 : s2 * expf(m2 - mn));
    m = mn;
    s = a + b;
}

// log-prob of a logit x in a row whose pair is (m, s): NaN anywhere in the row gives NaN, x == -inf gives -inf
__device__ __forceinline__ float row_logprob(float x, float m, float s) { return s != s ? s : (x == -INFINITY ? -INFINITY : (x - m) - logf(s)); }

// ------------------------------------------------------------------ the tile steps of a slice
static constexpr uint32_t ROW_THREADS = 256;
static constexpr uint32_t ROW_WAVES = ROW_THREADS / WAVE;
static constexpr uint32_t ROW_F4 = 4;                                  // float4 per thread per tile
static constexpr uint32_t ROW_TILE = ROW_THREADS * ROW_F4 * 4;         // 4096 logits per workgroup tile

// The slice kernels of wrk_score.hip and wrk_logprob.hip read a slice in register tiles of 16 floats per thread: per tile the loads
// (row_tile_load), the tile's max (row_tile_max), the tile's exp-sum -- ts += row_exp_term(x, max) over the tile in k, j order -- and
// row_merge into the thread's running pair; then the workgroup's pair in a fixed order, wave butterfly and the waves in index order,
// every step a row_merge.  The tile loop, the sum loop and the reduction's skeleton stay in each kernel: moved into a callee of any
// shape, the compiler orders the operands of the sum's additions differently (which changes the sign of a NaN result) and schedules
// the reduction differently, and these kernels are to compile to the code they had.

// index of x[k][0] of the calling thread's register tile at `base`
__device__ __forceinline__ uint32_t row_tile_index(uint32_t base, uint32_t k) { return base + (k * ROW_THREADS + threadIdx.x) * 4; }

// x[k][j] = logit row_tile_index(base, k) + j of `row`, -inf at or past `end` (VEC: 16-byte loads; the row is 16-byte aligned, base % 4 == 0)
template <bool VEC>
__device__ __forceinline__ void row_tile_load(const float* __restrict__ row, uint32_t base, uint32_t end, float (&x)[ROW_F4][4]) {
#pragma unroll
    for (uint32_t k = 0; k < ROW_F4; ++k) {
        const uint32_t i = row_tile_index(base, k);
        if (VEC && i + 3 < end) {
            const f32x4 q = *(const f32x4*)(row + i);
            x[k][0] = q.x; x[k][1] = q.y; x[k][2] = q.z; x[k][3] = q.w;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) x[k][j] = i + j < end ? row[i + j] : -INFINITY;
        }
    }
}

__device__ __forceinline__ float row_tile_max(const float (&x)[ROW_F4][4]) {
    float tm = -INFINITY;
#pragma unroll
    for (uint32_t k = 0; k < ROW_F4; ++k)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) tm = fmaxf(tm, x[k][j]);
    return tm;
}

// a logit's term of the tile's exp-sum: padding is -inf and adds 0; a NaN logit makes the sum NaN
__device__ __forceinline__ float row_exp_term(float y, float tm) { return y == -INFINITY ? 0.0f : expf(y - tm); }

// How score_rows and logprob_rows cut n rows of v logits: S = score_slices workgroups per row, each `len` logits (a multiple of 4), and
// whether the 16-byte loads apply
struct RowSlices { uint32_t S, len; bool vec; };
inline RowSlices row_slices(const float* logits, uint32_t v, uint32_t stride, uint32_t n, int num_cu) {
    const uint32_t S = score_slices(n, v, num_cu);
    const uint32_t len = ((v + S - 1) / S + 3) & ~3u;
    return RowSlices{S, len, stride % 4 == 0 && ((uintptr_t)logits & 15) == 0};
}

// ------------------------------------------------------------------ the gate
// whether row r's draw counts (RowGate, wrk_internal.h); read before anything else of the row
__device__ __forceinline__ bool row_counts(const RowGate& g, uint32_t r) { return !g.flag || g.flag[(size_t)r * g.stride] == g.eq; }

}  // namespace wrk
