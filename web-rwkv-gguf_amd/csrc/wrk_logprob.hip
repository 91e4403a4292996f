// Log-probs of chosen tokens and the N most likely alternatives, on the device for gfx950.  Per row x of f32 logits and chosen token y:
//   logprob         = (x_y - m) - log sum_i exp(x_i - m)     (m = the row max: row_logprob, which wrk_score.hip evaluates at the same slicing)
//   top_ids[j]      = the j-th token in the sampler's order (wrk_sample.hip): logit descending, ties by index ascending
//   top_logprobs[j] = the same expression at top_ids[j]
// for j < n = LogprobParam::num_top <= 20, which is device data: one captured step program serves any n.  A NaN anywhere makes every
// log-prob of the row NaN (ids unspecified); a logit of -inf has log-prob -inf and sorts after every finite logit, by index; entries
// j >= V are id 0xFFFFFFFF and -inf.  See DESIGN.md §7h.
//
// A row is split over S = score_slices workgroups of 256 threads and read in the tile steps that wrk_score.hip uses (wrk_rows_dev.h:
// register tiles of 16 floats per thread, wave butterfly, the four waves in index order), then the slices in slice order.  The order of
// the alternatives is the sampler's rank_key (wrk_rows_dev.h), so selection is integer work and ties cannot go wrong.  Each wave
// keeps its n best keys so far across lanes 0..n-1 (lane j: the j-th best) and folds a tile in with n rounds of "largest key strictly
// below the last chosen one" over the tile's register keys and the kept ones; a tile none of whose keys beats the n-th kept key is
// skipped.  No LDS, no barrier: a workgroup emits 4 x n candidates.  The second launch, one workgroup per row, picks the n best of the
// S x 4 x n candidates the same way (per wave, then wave 0 over the four waves' picks), merges the (max, sum) partials and writes the
// row.  Every reduction has a fixed order and there are no float atomics: the same (rows, V, stride, n) gives the same bits on every call.
#include "wrk_rows_dev.h"

namespace wrk {

static constexpr uint32_t LP_SLICE_KEYS = ROW_WAVES * LOGPROB_MAX_TOP;                     // candidate slots of one slice
static constexpr uint32_t LP_COMBINE_KEYS = (SCORE_MAX_SLICES * LP_SLICE_KEYS + ROW_THREADS - 1) / ROW_THREADS;   // per thread of the second launch
static constexpr uint32_t LP_NO_ID = 0xFFFFFFFFu;

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
__global__ void __launch_bounds__(ROW_THREADS) logprob_slice_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t len,
                                                                   const LogprobParam* __restrict__ par, LogprobPart* __restrict__ part,
                                                                   unsigned long long* __restrict__ keys) {
    __shared__ float sm_m[ROW_WAVES], sm_s[ROW_WAVES];
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = logits + (size_t)r * stride;
    const uint32_t n = par->num_top < LOGPROB_MAX_TOP ? par->num_top : LOGPROB_MAX_TOP;
    const uint32_t a = blockIdx.y * len;
    const uint32_t end = a + len < v ? a + len : v;
    float m = -INFINITY, s = 0.0f;
    unsigned long long keep = 0;
    for (uint32_t base = a; base < end; base += ROW_TILE) {
        float x[ROW_F4][4];
        row_tile_load<VEC>(row, base, end, x);
        const float tm = row_tile_max(x);
        float ts = 0.0f;
#pragma unroll
        for (uint32_t k = 0; k < ROW_F4; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) ts += row_exp_term(x[k][j], tm);
        row_merge(m, s, tm, ts);
        if (n) {
            unsigned long long key[ROW_F4 * 4];
#pragma unroll
            for (uint32_t k = 0; k < ROW_F4; ++k) {
                const uint32_t i = row_tile_index(base, k);
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) key[k * 4 + j] = i + j < end ? rank_key(row_norm(x[k][j]), i + j) : 0ull;
            }
            keep = wave_top(key, keep, n);
        }
    }
    if (lane < n) keys[((size_t)(r * gridDim.y + blockIdx.y) * ROW_WAVES + wid) * LOGPROB_MAX_TOP + lane] = keep;
    // workgroup reduction in a fixed order: wave butterfly, then the four waves in index order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, WAVE), os = __shfl_xor(s, o, WAVE);
        row_merge(m, s, om, os);
    }
    if (lane == 0) { sm_m[wid] = m; sm_s[wid] = s; }
    __syncthreads();
    if (tid != 0) return;
    m = sm_m[0]; s = sm_s[0];
    for (uint32_t w = 1; w < ROW_WAVES; ++w) row_merge(m, s, sm_m[w], sm_s[w]);
    part[(size_t)r * gridDim.y + blockIdx.y] = LogprobPart{m, s};
}

// one workgroup per row: the n best of the row's nslice * 4 * n candidates, the partials merged in slice order, the chosen token
// tokens[row], and the row's outputs at row (step ? *step : 0) * rows + row of the buffers `par` names
__global__ void __launch_bounds__(ROW_THREADS) logprob_combine_kernel(const float* __restrict__ logits, uint32_t v, uint32_t stride, uint32_t nslice,
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
            const uint32_t slot = tid + ROW_THREADS * u;
            key[u] = (slot < nslice * LP_SLICE_KEYS && slot % LOGPROB_MAX_TOP < n) ? keys[(size_t)r * nslice * LP_SLICE_KEYS + slot] : 0ull;
        }
        const unsigned long long top = wave_top(key, 0ull, n);
        if (lane < LOGPROB_MAX_TOP) cand[wid * LOGPROB_MAX_TOP + lane] = top;       // lanes >= n hold 0
    }
    __syncthreads();
    if (wid != 0) return;
    float m = sp[0].m, s = sp[0].s;
    for (uint32_t k = 1; k < nslice; ++k) row_merge(m, s, sp[k].m, sp[k].s);
    const size_t o = (size_t)(step ? *step : 0u) * gridDim.x + r;
    const bool room = o < par->cap_rows;         // a step past the buffers writes nothing
    const uint32_t y = tokens[r];
    if (lane == 0 && room) par->logprob[o] = y < v ? row_logprob(row[y], m, s) : NAN;
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
    par->top_logprobs[o * n + lane] = row_logprob(x, m, s);
}

int logprob_rows(hipStream_t st, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* tokens, const uint32_t* step,
                 const LogprobParam* par, LogprobPart* part, unsigned long long* keys, int num_cu) {
    if (n == 0) return 0;
    if (v == 0 || v > SAMPLE_MAX_VOCAB || stride < v) return -1;
    const RowSlices c = row_slices(logits, v, stride, n, num_cu);
    const dim3 grid(n, c.S);
    if (c.vec) logprob_slice_kernel<true><<<grid, ROW_THREADS, 0, st>>>(logits, v, stride, c.len, par, part, keys);
    else logprob_slice_kernel<false><<<grid, ROW_THREADS, 0, st>>>(logits, v, stride, c.len, par, part, keys);
    logprob_combine_kernel<<<n, ROW_THREADS, 0, st>>>(logits, v, stride, c.S, tokens, step, par, part, keys);
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
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_top_logprobs", wrk::SAMPLE_MAX_VOCAB);
    if (rc == WRK_OK) rc = wrk_score_check_targets(ctx, tokens, n, V);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rows_top = (size_t)n * (num_top ? num_top : 1);
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::LogprobParam)), o_tok = dev.add((size_t)n * 4), o_lp = dev.add((size_t)n * 4);
    const size_t o_ids = dev.add(rows_top * 4), o_tlp = dev.add(rows_top * 4);
    const size_t o_part = dev.add(wrk::logprob_part_bytes(n)), o_keys = dev.add(wrk::logprob_key_bytes(n));
    WRK_HIP(ctx, dev.alloc());
    const wrk::LogprobParam par{dev.at<float>(o_lp), dev.at<uint32_t>(o_ids), dev.at<float>(o_tlp), num_top, n};
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tok), tokens, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::logprob_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, dev.at<uint32_t>(o_tok), nullptr, dev.at<wrk::LogprobParam>(o_par),
                      dev.at<wrk::LogprobPart>(o_part), dev.at<unsigned long long>(o_keys), ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(logprob, par.logprob, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (num_top) {
        WRK_HIP(ctx, hipMemcpyAsync(top_ids, par.top_ids, rows_top * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(top_logprobs, par.top_logprobs, rows_top * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}
