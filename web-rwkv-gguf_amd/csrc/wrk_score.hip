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
#include "wrk_device.h"

namespace wrk {

static constexpr uint32_t SCORE_THREADS = 256;
static constexpr uint32_t SCORE_F4 = 4;                                    // float4 per thread per tile
static constexpr uint32_t SCORE_TILE = SCORE_THREADS * SCORE_F4 * 4;       // 4096 logits per workgroup tile
static constexpr uint32_t SCORE_MIN_SLICE = 2048;

uint32_t score_slices(uint32_t n, uint32_t v, int num_cu) {
    if (n == 0) return 1;
    const uint64_t want = ((uint64_t)4 * (uint32_t)(num_cu > 0 ? num_cu : 1) + n - 1) / n;     // about four workgroups per CU
    const uint64_t most = ((uint64_t)v + SCORE_MIN_SLICE - 1) / SCORE_MIN_SLICE;               // slices of at least 2048 logits
    uint64_t s = want < most ? want : most;
    if (s > SCORE_MAX_SLICES) s = SCORE_MAX_SLICES;
    return s < 1 ? 1 : (uint32_t)s;
}

// (m, s) <- the pair for the union of the two sets.  m is never NaN (fmaxf drops NaN operands); a NaN logit makes s NaN, which every later
// merge keeps.  s == 0 with m == -inf is the empty set.
__device__ __forceinline__ void score_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float a = s == 0.0f ? 0.0f : (m == mn ? s : s * expf(m - mn));
    const float b = s2 == 0.0f ? 0.0f : (m2 == mn ? s2 : s2 * expf(m2 - mn));
    m = mn;
    s = a + b;
}

__device__ __forceinline__ void score_finish(float xt, float m, float s, uint32_t gt, uint32_t eq, float* lp, uint32_t* rk) {
    *lp = s != s ? s : (xt == -INFINITY ? -INFINITY : (xt - m) - logf(s));
    *rk = gt + eq;
}

// grid (n, S): workgroup (row, slice) covers logits [slice * len, min((slice + 1) * len, v)) of its row; len % 4 == 0
template <bool VEC>
__global__ void __launch_bounds__(SCORE_THREADS) score_slice_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t len,
                                                                    const uint32_t* __restrict__ targets, ScorePart* __restrict__ part,
                                                                    float* __restrict__ logprob, uint32_t* __restrict__ rank) {
    __shared__ float sm_m[SCORE_THREADS / WAVE], sm_s[SCORE_THREADS / WAVE];
    __shared__ uint32_t sm_gt[SCORE_THREADS / WAVE], sm_eq[SCORE_THREADS / WAVE];
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const float* row = logits + (size_t)r * stride;
    const uint32_t t = targets[r];
    const float xt = row[t];
    const uint32_t a = blockIdx.y * len;
    const uint32_t end = a + len < v ? a + len : v;
    const uint32_t lim = t < end ? t : end;       // the equal-before count covers [a, lim)
    float m = -INFINITY, s = 0.0f;
    uint32_t gt = 0, eq = 0;
    for (uint32_t base = a; base < end; base += SCORE_TILE) {
        float x[SCORE_F4][4];
#pragma unroll
        for (uint32_t k = 0; k < SCORE_F4; ++k) {
            const uint32_t i = base + (k * SCORE_THREADS + tid) * 4;
            if (VEC && i + 3 < end) {
                const f32x4 q = *(const f32x4*)(row + i);
                x[k][0] = q.x; x[k][1] = q.y; x[k][2] = q.z; x[k][3] = q.w;
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) x[k][j] = i + j < end ? row[i + j] : -INFINITY;
            }
        }
        float tm = -INFINITY;
#pragma unroll
        for (uint32_t k = 0; k < SCORE_F4; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) tm = fmaxf(tm, x[k][j]);
        float ts = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < SCORE_F4; ++k) {
            const uint32_t i = base + (k * SCORE_THREADS + tid) * 4;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const float y = x[k][j];
                ts += y == -INFINITY ? 0.0f : expf(y - tm);      // padding is -inf; a NaN logit makes ts NaN
                gt += y > xt ? 1u : 0u;
                eq += (y == xt && i + j < lim) ? 1u : 0u;
            }
        }
        score_merge(m, s, tm, ts);
    }
    // workgroup reduction in a fixed order: wave butterfly, then the four waves in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, WAVE), os = __shfl_xor(s, o, WAVE);
        score_merge(m, s, om, os);
        gt += __shfl_xor(gt, o, WAVE);
        eq += __shfl_xor(eq, o, WAVE);
    }
    if ((tid & 63) == 0) { sm_m[tid >> 6] = m; sm_s[tid >> 6] = s; sm_gt[tid >> 6] = gt; sm_eq[tid >> 6] = eq; }
    __syncthreads();
    if (tid != 0) return;
    m = sm_m[0]; s = sm_s[0]; gt = sm_gt[0]; eq = sm_eq[0];
    for (uint32_t w = 1; w < SCORE_THREADS / WAVE; ++w) { score_merge(m, s, sm_m[w], sm_s[w]); gt += sm_gt[w]; eq += sm_eq[w]; }
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
    for (uint32_t k = 1; k < nslice; ++k) { score_merge(m, s, sp[w][k].m, sp[w][k].s); gt += sp[w][k].gt; eq += sp[w][k].eq; }
    score_finish(xt, m, s, gt, eq, logprob + r, rank + r);
}

int score_rows(hipStream_t st, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* targets, ScorePart* part,
               float* logprob, uint32_t* rank, int num_cu) {
    if (n == 0) return 0;
    if (v == 0 || stride < v) return -1;
    const uint32_t S = score_slices(n, v, num_cu);
    uint32_t len = (v + S - 1) / S;
    len = (len + 3) & ~3u;
    const dim3 grid(n, S);
    if (stride % 4 == 0 && ((uintptr_t)logits & 15) == 0)
        score_slice_kernel<true><<<grid, SCORE_THREADS, 0, st>>>(logits, v, stride, len, targets, part, logprob, rank);
    else score_slice_kernel<false><<<grid, SCORE_THREADS, 0, st>>>(logits, v, stride, len, targets, part, logprob, rank);
    if (S > 1) score_combine_kernel<<<(n + 256 / WAVE - 1) / (256 / WAVE), 256, 0, st>>>(logits, stride, n, S, targets, part, logprob, rank);
    return 0;
}

}  // namespace wrk

int32_t wrk_score_scratch::ensure(wrk_ctx* ctx, uint32_t n, bool* grown) {
    *grown = false;
    if (n <= cap && buf) return WRK_OK;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (buf) hipFree(buf);
    buf = nullptr;
    cap = 0;
    *grown = true;
    const size_t o_lp = ((size_t)n * 4 + 255) & ~(size_t)255, o_rk = o_lp + (((size_t)n * 4 + 255) & ~(size_t)255);
    const size_t o_part = o_rk + (((size_t)n * 4 + 255) & ~(size_t)255);
    WRK_HIP(ctx, hipMalloc(&buf, o_part + (size_t)n * wrk::SCORE_MAX_SLICES * sizeof(wrk::ScorePart)));
    char* b = (char*)buf;
    targets = (uint32_t*)b; logprob = (float*)(b + o_lp); rank = (uint32_t*)(b + o_rk); part = (wrk::ScorePart*)(b + o_part);
    cap = n;
    return WRK_OK;
}

void wrk_score_scratch::release() {
    if (buf) hipFree(buf);
    buf = nullptr;
    cap = 0;
}

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
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_score_logits is blocking: not inside a capture");
    WRK_ARG(ctx, V >= 1 && stride >= V, "num_vocab %u / row_stride %u", V, stride);
    WRK_ARG(ctx, ((size_t)(n - 1) * stride + V) * 4 <= logits->bytes, "%u rows of stride %u exceed the buffer of %zu bytes", n, stride,
            logits->bytes);
    const int32_t rc = wrk_score_check_targets(ctx, targets, n, V);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_score_scratch sc;
    bool grown = false;
    const int32_t rc2 = sc.ensure(ctx, n, &grown);
    if (rc2 != WRK_OK) return rc2;
    struct Free { wrk_score_scratch* p; ~Free() { p->release(); } } guard{&sc};
    WRK_HIP(ctx, hipMemcpyAsync(sc.targets, targets, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::score_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, sc.targets, sc.part, sc.logprob, sc.rank, ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(logprob, sc.logprob, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(rank, sc.rank, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}
