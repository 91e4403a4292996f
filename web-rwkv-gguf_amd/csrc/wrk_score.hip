// Sequence scoring on the device for gfx950: per row of f32 logits and a target token t,
//   logprob = x_t - (m + log sum_i exp(x_i - m))      (m = the row max; computed as (x_t - m) - log(sum))
//   rank    = #{i : x_i > x_t} + #{i < t : x_i == x_t}  (0 exactly when t is argmax_rows' answer, the first index of the maximum)
// A NaN anywhere gives logprob NaN (rank unspecified); a target logit of -inf gives -inf.  See DESIGN.md §7b.
//
// One row is split into S slices (S from n, V and num_cu only, score_slices) over S workgroups, so that a few rows still spread over the
// GPU.  A workgroup reads its slice once, in register tiles of 16 floats per thread: the tile's max first, then the tile's exp-sum from the
// registers, merged into a running (max, sum) pair.  Per-slice partials (max, sum, count_greater, count_equal_before) go to scratch and a
// second launch combines them in slice order; with S == 1 the first launch finishes the row itself.  Every reduction has a fixed order and
// there are no float atomics: the same (n, V, stride) gives the same bits on every replay.
#include "wrk_rows_dev.h"

namespace wrk {

static constexpr uint32_t SCORE_MIN_SLICE = 2048;

uint32_t score_slices(uint32_t n, uint32_t v, int num_cu) {
    if (n == 0) return 1;
    const uint64_t want = ((uint64_t)4 * (uint32_t)(num_cu > 0 ? num_cu : 1) + n - 1) / n;     // about four workgroups per CU
    const uint64_t most = ((uint64_t)v + SCORE_MIN_SLICE - 1) / SCORE_MIN_SLICE;               // slices of at least 2048 logits
    uint64_t s = want < most ? want : most;
    if (s > SCORE_MAX_SLICES) s = SCORE_MAX_SLICES;
    return s < 1 ? 1 : (uint32_t)s;
}

__device__ __forceinline__ void score_finish(float xt, float m, float s, uint32_t gt, uint32_t eq, float* lp, uint32_t* rk) {
    *lp = row_logprob(xt, m, s);
    *rk = gt + eq;
}

// grid (n, S): workgroup (row, slice) covers logits [slice * len, min((slice + 1) * len, v)) of its row; len % 4 == 0
template <bool VEC>
__global__ void __launch_bounds__(ROW_THREADS) score_slice_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t len,
                                                                  const uint32_t* __restrict__ targets, ScorePart* __restrict__ part,
                                                                  float* __restrict__ logprob, uint32_t* __restrict__ rank) {
    __shared__ float sm_m[ROW_WAVES], sm_s[ROW_WAVES];
    __shared__ uint32_t sm_gt[ROW_WAVES], sm_eq[ROW_WAVES];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (size_t)r * stride;
    const uint32_t t = targets[r];
    const float xt = row[t];
    const uint32_t a = blockIdx.y * len;
    const uint32_t end = a + len < v ? a + len : v;
    const uint32_t lim = t < end ? t : end;       // the equal-before count covers [a, lim)
    float m = -INFINITY, s = 0.0f;
    uint32_t gt = 0, eq = 0;
    for (uint32_t base = a; base < end; base += ROW_TILE) {
        float x[ROW_F4][4];
        row_tile_load<VEC>(row, base, end, x);
        const float tm = row_tile_max(x);
        float ts = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < ROW_F4; ++k) {
            const uint32_t i = row_tile_index(base, k);
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const float y = x[k][j];
                ts += row_exp_term(y, tm);
                gt += y > xt ? 1u : 0u;
                eq += (y == xt && i + j < lim) ? 1u : 0u;
            }
        }
        row_merge(m, s, tm, ts);
    }
    // workgroup reduction in a fixed order: wave butterfly, then the four waves in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, WAVE), os = __shfl_xor(s, o, WAVE);
        row_merge(m, s, om, os);
        gt += __shfl_xor(gt, o, WAVE);
        eq += __shfl_xor(eq, o, WAVE);
    }
    if ((tid & 63) == 0) { sm_m[tid >> 6] = m; sm_s[tid >> 6] = s; sm_gt[tid >> 6] = gt; sm_eq[tid >> 6] = eq; }
    __syncthreads();
    if (tid != 0) return;
    m = sm_m[0]; s = sm_s[0]; gt = sm_gt[0]; eq = sm_eq[0];
    for (uint32_t w = 1; w < ROW_WAVES; ++w) { row_merge(m, s, sm_m[w], sm_s[w]); gt += sm_gt[w]; eq += sm_eq[w]; }
    if (gridDim.y == 1) score_finish(xt, m, s, gt, eq, logprob + r, rank + r);
    else part[(size_t)r * gridDim.y + blockIdx.y] = ScorePart{m, s, gt, eq};
}

// one wave per row: lane k loads slice k's partial (one memory round trip for all of them), lane 0 merges them in slice order from LDS
__global__ void __launch_bounds__(256) score_combine_kernel(const float* __restrict__ logits, uint32_t stride, uint32_t n, uint32_t nslice,
                                                            const uint32_t* __restrict__ targets, const ScorePart* __restrict__ part,
                                                            float* __restrict__ logprob, uint32_t* __restrict__ rank) {
    __shared__ ScorePart sp[256 / WAVE][SCORE_MAX_SLICES];
    const uint32_t w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const uint32_t r = blockIdx.x * (256 / WAVE) + w;
    const bool live = r < n;
    if (live && lane < nslice) sp[w][lane] = part[(size_t)r * nslice + lane];
    float xt = 0.0f;
    if (live && lane == 0) xt = logits[(size_t)r * stride + targets[r]];
    __syncthreads();
    if (!live || lane != 0) return;
    float m = sp[w][0].m, s = sp[w][0].s;
    uint32_t gt = sp[w][0].gt, eq = sp[w][0].eq;
    for (uint32_t k = 1; k < nslice; ++k) { row_merge(m, s, sp[w][k].m, sp[w][k].s); gt += sp[w][k].gt; eq += sp[w][k].eq; }
    score_finish(xt, m, s, gt, eq, logprob + r, rank + r);
}

int score_rows(hipStream_t st, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* targets, ScorePart* part,
               float* logprob, uint32_t* rank, int num_cu) {
    if (n == 0) return 0;
    if (v == 0 || stride < v) return -1;
    const RowSlices c = row_slices(logits, v, stride, n, num_cu);
    const uint32_t S = c.S;
    const dim3 grid(n, S);
    if (c.vec) score_slice_kernel<true><<<grid, ROW_THREADS, 0, st>>>(logits, v, stride, c.len, targets, part, logprob, rank);
    else score_slice_kernel<false><<<grid, ROW_THREADS, 0, st>>>(logits, v, stride, c.len, targets, part, logprob, rank);
    if (S > 1) score_combine_kernel<<<(n + 256 / WAVE - 1) / (256 / WAVE), 256, 0, st>>>(logits, stride, n, S, targets, part, logprob, rank);
    return 0;
}

}  // namespace wrk

int32_t wrk_score_check_targets(wrk_ctx* ctx, const uint32_t* targets, uint32_t n, uint32_t V) {
    WRK_ARG(ctx, n == 0 || targets, "targets required");
    for (uint32_t h = 0; h < n; ++h) WRK_ARG(ctx, targets[h] < V, "target %u: id %u >= vocab %u", h, targets[h], V);
    return WRK_OK;
}

extern "C" int32_t wrk_score_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const uint32_t* targets,
                                    float* logprob, uint32_t* rank) {
    if (!ctx || !logits) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    if (n == 0) return WRK_OK;
    WRK_ARG(ctx, logprob && rank, "logprob and rank are required");
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_score_logits", 0);
    if (rc == WRK_OK) rc = wrk_score_check_targets(ctx, targets, n, V);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_tg = dev.add((size_t)n * 4), o_lp = dev.add((size_t)n * 4), o_rk = dev.add((size_t)n * 4);
    const size_t o_part = dev.add((size_t)n * wrk::SCORE_MAX_SLICES * sizeof(wrk::ScorePart));
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tg), targets, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::score_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, dev.at<uint32_t>(o_tg), dev.at<wrk::ScorePart>(o_part), dev.at<float>(o_lp),
                    dev.at<uint32_t>(o_rk), ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(logprob, dev.at<char>(o_lp), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(rank, dev.at<char>(o_rk), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}
