// Log-probs of chosen tokens and the N most likely alternatives, on the device for gfx950.  Per row x of f32 logits and chosen token y:
//   logprob         = (x_y - m) - log sum_i exp(x_i - m)     (m = the row max: wrk_score.hip's expression, bit for bit at the same slicing)
//   top_ids[j]      = the j-th token in the sampler's order (wrk_sample.hip): logit descending, ties by index ascending
//   top_logprobs[j] = the same expression at top_ids[j]
// for j < n = LogprobParam::num_top <= 20, which is device data: one captured step program serves any n.  A NaN anywhere makes every
// log-prob of the row NaN (ids unspecified); a logit of -inf has log-prob -inf and sorts after every finite logit, by index; entries
// j >= V are id 0xFFFFFFFF and -inf.  See DESIGN.md §7h.
//
// A row is split over S = score_slices workgroups of 256 threads, as in wrk_score.hip and with its (max, sum) arithmetic: register tiles
// of 16 floats per thread, wave butterfly, the four waves in index order, then the slices in slice order.  The order of the alternatives
// is the sampler's unique 52-bit key monotone(logit) << 20 | ~index, so selection is integer work and ties cannot go wrong.  Each wave
// keeps its n best keys so far across lanes 0..n-1 (lane j: the j-th best) and folds a tile in with n rounds of "largest key strictly
// below the last chosen one" over the tile's register keys and the kept ones; a tile none of whose keys beats the n-th kept key is
// skipped.  No LDS, no barrier: a workgroup emits 4 x n candidates.  The second launch, one workgroup per row, picks the n best of the
// S x 4 x n candidates the same way (per wave, then wave 0 over the four waves' picks), merges the (max, sum) partials and writes the
// row.  Every reduction has a fixed order and there are no float atomics: the same (rows, V, stride, n) gives the same bits on every call.
#include "wrk_device.h"

namespace wrk {

static constexpr uint32_t LP_THREADS = 256;
static constexpr uint32_t LP_WAVES = LP_THREADS / WAVE;
static constexpr uint32_t LP_F4 = 4;                                // float4 per thread per tile
static constexpr uint32_t LP_TILE = LP_THREADS * LP_F4 * 4;         // 4096 logits per workgroup tile (wrk_score.hip's)
static constexpr uint32_t LP_SLICE_KEYS = LP_WAVES * LOGPROB_MAX_TOP;                      // candidate slots of one slice
static constexpr uint32_t LP_COMBINE_KEYS = (SCORE_MAX_SLICES * LP_SLICE_KEYS + LP_THREADS - 1) / LP_THREADS;   // per thread of the second launch
static constexpr uint32_t LP_NO_ID = 0xFFFFFFFFu;

// wrk_score.hip's score_merge: (m, s) <- the pair for the union of the two sets
__device__ __forceinline__ void lp_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    const float a = s == 0.0f ? 0.0f : (m == mn ? s : s * expf(m - mn));
    const float b = s2 == 0.0f ? 0.0f : (m2 == mn ? s2 : s2 * expf(m2 - mn));
    m = mn;
    s = a + b;
}

// wrk_score.hip's score_finish
__device__ __forceinline__ float lp_finish(float x, float m, float s) { return s != s ? s : (x == -INFINITY ? -INFINITY : (x - m) - logf(s)); }

// the sampler's rank_key on its normalised logit (NaN counts as -inf, -0 as +0); never 0 for a token, 0 is "none"
__device__ __forceinline__ unsigned long long lp_key(float l, uint32_t i) {
    l = l != l ? -INFINITY : l + 0.0f;
    uint32_t b = __float_as_uint(l);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 20) | (0xFFFFFu - i);
}

// The n largest of the wave's keys k[0..NK) and `keep` (lanes 0..n-1: the n best so far, descending; 0 elsewhere), returned the same way.
// All 64 lanes call it; n >= 1; keys are unique or 0
template <int NK>
__device__ __forceinline__ unsigned long long wave_top(const unsigned long long (&k)[NK], unsigned long long keep, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long floor_key = __shfl(keep, (int)(n - 1), WAVE);      // 0 while fewer than n are kept
    unsigned long long best = 0;
#pragma unroll
    for (int u = 0; u < NK; ++u) best = k[u] > best ? k[u] : best;
    if (__ballot(best > floor_key) == 0) return keep;
    unsigned long long last = ~0ull, out = 0;
    for (uint32_t r = 0; r < n; ++r) {
        unsigned long long c = keep < last ? keep : 0;
#pragma unroll
        for (int u = 0; u < NK; ++u) c = (k[u] < last && k[u] > c) ? k[u] : c;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long t = __shfl_xor(c, o, WAVE);
            c = t > c ? t : c;
        }
        if (c == 0) break;          // uniform: fewer than n keys in all
        if (lane == r) out = c;
        last = c;
    }
    return out;
}

// grid (rows, S): workgroup (row, slice) covers logits [slice * len, min((slice + 1) * len, v)) of its row; len % 4 == 0.  Leaves
// part[row * S + slice] and, with n > 0, wave w's n best keys at keys[((row * S + slice) * 4 + w) * 20 ..]
template <bool VEC>
__global__ void __launch_bounds__(LP_THREADS) logprob_slice_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t len,
                                                                   const LogprobParam* __restrict__ par, LogprobPart* __restrict__ part,
                                                                   unsigned long long* __restrict__ keys) {
    __shared__ float sm_m[LP_WAVES], sm_s[LP_WAVES];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = logits + (size_t)r * stride;
    const uint32_t n = par->num_top < LOGPROB_MAX_TOP ? par->num_top : LOGPROB_MAX_TOP;
    const uint32_t a = blockIdx.y * len;
    const uint32_t end = a + len < v ? a + len : v;
    float m = -INFINITY, s = 0.0f;
    unsigned long long keep = 0;
    for (uint32_t base = a; base < end; base += LP_TILE) {
        float x[LP_F4][4];
#pragma unroll
        for (uint32_t k = 0; k < LP_F4; ++k) {
            const uint32_t i = base + (k * LP_THREADS + tid) * 4;
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
        for (uint32_t k = 0; k < LP_F4; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) tm = fmaxf(tm, x[k][j]);
        float ts = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < LP_F4; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const float y = x[k][j];
                ts += y == -INFINITY ? 0.0f : expf(y - tm);     // padding is -inf; a NaN logit makes ts NaN
            }
        lp_merge(m, s, tm, ts);
        if (n) {
            unsigned long long key[LP_F4 * 4];
#pragma unroll
            for (uint32_t k = 0; k < LP_F4; ++k) {
                const uint32_t i = base + (k * LP_THREADS + tid) * 4;
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) key[k * 4 + j] = i + j < end ? lp_key(x[k][j], i + j) : 0ull;
            }
            keep = wave_top(key, keep, n);
        }
    }
    if (lane < n) keys[((size_t)(r * gridDim.y + blockIdx.y) * LP_WAVES + wid) * LOGPROB_MAX_TOP + lane] = keep;
    // workgroup reduction in wrk_score.hip's order: wave butterfly, then the four waves in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, WAVE), os = __shfl_xor(s, o, WAVE);
        lp_merge(m, s, om, os);
    }
    if (lane == 0) { sm_m[wid] = m; sm_s[wid] = s; }
    __syncthreads();
    if (tid != 0) return;
    m = sm_m[0]; s = sm_s[0];
    for (uint32_t w = 1; w < LP_WAVES; ++w) lp_merge(m, s, sm_m[w], sm_s[w]);
    part[(size_t)r * gridDim.y + blockIdx.y] = LogprobPart{m, s};
}

// one workgroup per row: the n best of the row's nslice * 4 * n candidates, the partials merged in slice order, the chosen token
// tokens[row], and the row's outputs at row (step ? *step : 0) * rows + row of the buffers `par` names
__global__ void __launch_bounds__(LP_THREADS) logprob_combine_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t nslice,
                                                                     const uint32_t* __restrict__ tokens, const uint32_t* __restrict__ step,
                                                                     const LogprobParam* __restrict__ par, const LogprobPart* __restrict__ part,
                                                                     const unsigned long long* __restrict__ keys) {
    __shared__ LogprobPart sp[SCORE_MAX_SLICES];
    __shared__ unsigned long long cand[LP_SLICE_KEYS];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = logits + (size_t)r * stride;
    const uint32_t n = par->num_top < LOGPROB_MAX_TOP ? par->num_top : LOGPROB_MAX_TOP;
    if (tid < nslice) sp[tid] = part[(size_t)r * nslice + tid];
    if (n) {
        unsigned long long key[LP_COMBINE_KEYS];
#pragma unroll
        for (uint32_t u = 0; u < LP_COMBINE_KEYS; ++u) {
            const uint32_t slot = tid + LP_THREADS * u;
            key[u] = (slot < nslice * LP_SLICE_KEYS && slot % LOGPROB_MAX_TOP < n) ? keys[(size_t)r * nslice * LP_SLICE_KEYS + slot] : 0ull;
        }
        const unsigned long long top = wave_top(key, 0ull, n);
        if (lane < LOGPROB_MAX_TOP) cand[wid * LOGPROB_MAX_TOP + lane] = top;       // lanes >= n hold 0
    }
    __syncthreads();
    if (wid != 0) return;
    float m = sp[0].m, s = sp[0].s;
    for (uint32_t k = 1; k < nslice; ++k) lp_merge(m, s, sp[k].m, sp[k].s);
    const size_t o = (size_t)(step ? *step : 0u) * gridDim.x + r;
    const bool room = o < par->cap_rows;         // a step past the buffers writes nothing
    const uint32_t y = tokens[r];
    if (lane == 0 && room) par->logprob[o] = y < v ? lp_finish(row[y], m, s) : NAN;
    if (!n) return;
    unsigned long long key[2];
    key[0] = cand[lane];
    key[1] = lane + WAVE < LP_SLICE_KEYS ? cand[lane + WAVE] : 0ull;
    const unsigned long long top = wave_top(key, 0ull, n);
    if (lane >= n || !room) return;
    const uint32_t id = top ? 0xFFFFFu - (uint32_t)(top & 0xFFFFFu) : LP_NO_ID;
    // the logit as it is in memory, as for the chosen token: when y is top_ids[0] the two log-probs have the same bits
    const float x = top ? row[id] : -INFINITY;
    par->top_ids[o * n + lane] = id;
    par->top_logprobs[o * n + lane] = lp_finish(x, m, s);
}

int logprob_rows(hipStream_t st, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* tokens, const uint32_t* step,
                 const LogprobParam* par, LogprobPart* part, unsigned long long* keys, int num_cu) {
    if (n == 0) return 0;
    if (v == 0 || v > SAMPLE_MAX_VOCAB || stride < v) return -1;
    const uint32_t S = score_slices(n, v, num_cu);
    uint32_t len = (v + S - 1) / S;
    len = (len + 3) & ~3u;
    const dim3 grid(n, S);
    if (stride % 4 == 0 && ((uintptr_t)logits & 15) == 0)
        logprob_slice_kernel<true><<<grid, LP_THREADS, 0, st>>>(logits, v, stride, len, par, part, keys);
    else logprob_slice_kernel<false><<<grid, LP_THREADS, 0, st>>>(logits, v, stride, len, par, part, keys);
    logprob_combine_kernel<<<n, LP_THREADS, 0, st>>>(logits, v, stride, S, tokens, step, par, part, keys);
    return 0;
}

}  // namespace wrk

extern "C" int32_t wrk_top_logprobs(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const uint32_t* tokens,
                                    uint32_t num_top, float* logprob, uint32_t* top_ids, float* top_logprobs) {
    if (!ctx || !logits) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, num_top <= WRK_MAX_TOP_LOGPROBS, "num_top %u: at most %u", num_top, (uint32_t)WRK_MAX_TOP_LOGPROBS);
    if (n == 0) return WRK_OK;
    WRK_ARG(ctx, logprob, "logprob is required");
    WRK_ARG(ctx, num_top == 0 || (top_ids && top_logprobs), "top_ids and top_logprobs are required with num_top > 0");
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_top_logprobs is blocking: not inside a capture");
    WRK_ARG(ctx, V >= 1 && stride >= V, "num_vocab %u / row_stride %u", V, stride);
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, ((size_t)(n - 1) * stride + V) * 4 <= logits->bytes, "%u rows of stride %u exceed the buffer of %zu bytes", n, stride,
            logits->bytes);
    const int32_t rc = wrk_score_check_targets(ctx, tokens, n, V);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t rows_top = (size_t)n * (num_top ? num_top : 1);
    const size_t o_tok = up(sizeof(wrk::LogprobParam)), o_lp = o_tok + up((size_t)n * 4), o_ids = o_lp + up((size_t)n * 4);
    const size_t o_tlp = o_ids + up(rows_top * 4), o_part = o_tlp + up(rows_top * 4);
    const size_t o_keys = o_part + up(wrk::logprob_part_bytes(n)), total = o_keys + wrk::logprob_key_bytes(n);
    char* dev = nullptr;
    WRK_HIP(ctx, hipMalloc((void**)&dev, total));
    struct Free { char* p; ~Free() { hipFree(p); } } guard{dev};
    const wrk::LogprobParam par{(float*)(dev + o_lp), (uint32_t*)(dev + o_ids), (float*)(dev + o_tlp), num_top, n};
    WRK_HIP(ctx, hipMemcpyAsync(dev, &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev + o_tok, tokens, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::logprob_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, (const uint32_t*)(dev + o_tok), nullptr, (const wrk::LogprobParam*)dev,
                      (wrk::LogprobPart*)(dev + o_part), (unsigned long long*)(dev + o_keys), ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(logprob, dev + o_lp, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (num_top) {
        WRK_HIP(ctx, hipMemcpyAsync(top_ids, dev + o_ids, rows_top * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(top_logprobs, dev + o_tlp, rows_top * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}
