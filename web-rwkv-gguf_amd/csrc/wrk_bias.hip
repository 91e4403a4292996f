// Logit bias on the device for gfx950: per-row sparse additive biases and bans (ai00's `bias`, llama.cpp's --logit-bias, the first link
// of its sampler chain, vLLM's / the OpenAI interfaces' logit_bias).  See DESIGN.md §7p.
//
// A wrk_logit_bias holds num_sets bias sets over one vocabulary as one CSR: set s is the pairs (ids[e], values[e]) for e in
// [offsets[s], offsets[s + 1]), stored sorted by id, every id once.  A row with set s becomes
//   x'[t] = -inf (its bits)        t in the set with value -inf: a ban, whatever x[t] is -- not x + (-inf), NaN for x = +inf
//   x'[t] = x[t] + v               t in the set with a finite value v: one f32 addition
//   x'[t] = x[t], bits unchanged   everywhere else (NaN payloads and -0 included); a row whose set is WRK_BIAS_NONE: all of it
//
//   bias_rows   grid (spans of BIAS_SPAN tokens, rows).  A workgroup first copies its span from `in` to `out` (skipped in place), then,
//               behind a barrier, finds by two binary searches the entries of the row's set whose ids fall inside its span and applies
//               them, one thread per entry: it reads x from `in` and stores the result to `out`.  No workgroup writes outside its span,
//               so there are no hazards between workgroups and no atomics; a set of a few entries costs two searches per workgroup, one of
//               tens of thousands O(V + E) over the row, not O(spans x E).
//
// Everything of the object reaches the kernel through a BiasParam block in device memory, so a captured step program holds no table
// pointer of its own.  Plain vector loads and stores only; no kernel waits on another.
#include "wrk_rows_dev.h"
#include "wrk_runner.h" // wrk_buf_write_raw

#include <algorithm>
#include <numeric>

namespace wrk {

static constexpr uint32_t BIAS_THREADS = 256;
static constexpr uint32_t BIAS_TILE = BIAS_THREADS * 4;        // tokens of one tile: 4 per thread
static constexpr uint32_t BIAS_TILES = 4;                      // tiles per workgroup
static constexpr uint32_t BIAS_SPAN = BIAS_TILE * BIAS_TILES;  // tokens per workgroup
static constexpr uint32_t BIAS_NEG_INF_BITS = 0xFF800000u;

// first e in [lo, hi) with ids[e] >= key (hi if none); ids ascending in the range
__device__ __forceinline__ uint32_t bias_lower_bound(const uint32_t* __restrict__ ids, uint32_t lo, uint32_t hi, uint32_t key) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// VEC: every row of in / out starts 16-byte aligned and v % 4 == 0, so thread tid owns the 4 tokens at a + 4 * tid of each tile; otherwise
// it owns a + tid + 256 * j (j < 4), one coalesced scalar access each.  The copy moves logits as u32: no float operation touches them.
// COPY false: in == out, nothing to copy.  The apply phase reads `in`, which nothing writes when it is another buffer, and in place
// every element of a span is read and written by the one thread that owns its entry
template <bool VEC, bool COPY>
__global__ void __launch_bounds__(BIAS_THREADS) bias_rows_kernel(const uint32_t* in, uint32_t v, uint32_t in_stride,
                                                                 const BiasParam* __restrict__ par, uint32_t* out, uint32_t out_stride) {
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const uint32_t* x = in + (size_t)r * in_stride;
    uint32_t* y = out + (size_t)r * out_stride;
    const uint32_t a0 = blockIdx.x * BIAS_SPAN;
    if (COPY) {
        if (VEC) {
            u32x4 xv[BIAS_TILES];
#pragma unroll
            for (uint32_t k = 0; k < BIAS_TILES; ++k) {
                const uint32_t i = a0 + k * BIAS_TILE + tid * 4;
                if (i < v) xv[k] = *(const u32x4*)(x + i);
            }
#pragma unroll
            for (uint32_t k = 0; k < BIAS_TILES; ++k) {
                const uint32_t i = a0 + k * BIAS_TILE + tid * 4;
                if (i < v) *(u32x4*)(y + i) = xv[k];
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < BIAS_TILES; ++k)
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t i = a0 + k * BIAS_TILE + j * BIAS_THREADS + tid;
                    if (i < v) y[i] = x[i];
                }
        }
        __syncthreads();        // the span's copy is in `out` before an entry's result overwrites its element
    }
    const BiasParam p = *par;
    const uint32_t set = p.sets[r];
    if (set == WRK_BIAS_NONE) return;
    const uint32_t lo = p.offsets[set], hi = p.offsets[set + 1];
    if (lo == hi) return;
    const uint32_t a1 = a0 + BIAS_SPAN < v ? a0 + BIAS_SPAN : v;
    const uint32_t first = bias_lower_bound(p.ids, lo, hi, a0), last = bias_lower_bound(p.ids, first, hi, a1);
    for (uint32_t e = first + tid; e < last; e += BIAS_THREADS) {
        const uint32_t t = p.ids[e];
        const float b = p.values[e];
        y[t] = b == -INFINITY ? BIAS_NEG_INF_BITS : __float_as_uint(__uint_as_float(x[t]) + b);
    }
}

void bias_rows(hipStream_t s, const float* in, uint32_t v, uint32_t in_stride, uint32_t n, const BiasParam* par, float* out, uint32_t out_stride) {
    if (n == 0 || v == 0) return;
    const dim3 grid((v + BIAS_SPAN - 1) / BIAS_SPAN, n);
    const uint32_t* src = (const uint32_t*)in;
    uint32_t* dst = (uint32_t*)out;
    if (in == out && in_stride == out_stride) {
        bias_rows_kernel<false, false><<<grid, BIAS_THREADS, 0, s>>>(src, v, in_stride, par, dst, out_stride);
        return;
    }
    if (v % 4 == 0 && in_stride % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
        bias_rows_kernel<true, true><<<grid, BIAS_THREADS, 0, s>>>(src, v, in_stride, par, dst, out_stride);
    else bias_rows_kernel<false, true><<<grid, BIAS_THREADS, 0, s>>>(src, v, in_stride, par, dst, out_stride);
}

}  // namespace wrk

wrk::BiasParam wrk_logit_bias::param(const uint32_t* sets) const { return wrk::BiasParam{offsets, ids, values, sets}; }

int32_t wrk_bias_pack(wrk_ctx* ctx, const wrk_logit_bias* lb, const uint32_t* set, uint32_t n, uint32_t V, std::vector<uint32_t>& out) {
    WRK_ARG(ctx, lb, "logit bias required");
    WRK_ARG(ctx, lb->ctx == ctx, "the logit bias belongs to another context");
    WRK_ARG(ctx, lb->num_vocab == V, "logit bias of %u tokens, logits of %u", lb->num_vocab, V);
    out.assign(n, 0u);
    for (uint32_t r = 0; r < n && set; ++r) {
        WRK_ARG(ctx, set[r] < lb->num_sets || set[r] == WRK_BIAS_NONE, "bias_set[%u] = %u: neither a set (< %u) nor WRK_BIAS_NONE", r, set[r],
                lb->num_sets);
        out[r] = set[r];
    }
    return WRK_OK;
}

extern "C" {

int32_t wrk_logit_bias_create(wrk_ctx* ctx, uint32_t V, uint32_t S, const uint32_t* set_offsets, const uint32_t* ids, const float* values,
                              wrk_logit_bias** out) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, S >= 1 && S <= WRK_MAX_BIAS_SETS, "num_sets %u: must be in [1, %u]", S, (uint32_t)WRK_MAX_BIAS_SETS);
    WRK_ARG(ctx, set_offsets && ids && values, "set_offsets, ids and values are required");
    WRK_ARG(ctx, set_offsets[0] == 0, "set_offsets[0] = %u: must be 0", set_offsets[0]);
    for (uint32_t s = 0; s < S; ++s) {
        WRK_ARG(ctx, set_offsets[s + 1] >= set_offsets[s], "set_offsets[%u] = %u decreases", s + 1, set_offsets[s + 1]);
        WRK_ARG(ctx, set_offsets[s + 1] - set_offsets[s] <= V, "set %u: %u entries for %u tokens", s, set_offsets[s + 1] - set_offsets[s], V);
    }
    // every set validated as it is copied, sorted by id (the kernel finds a span's entries by binary search): nothing is sized by, and
    // nothing of the caller's arrays is read at, an offset that has not been checked
    std::vector<uint32_t> sid, order;
    std::vector<float> sval;
    for (uint32_t s = 0; s < S; ++s) {
        const uint32_t lo = set_offsets[s], cnt = set_offsets[s + 1] - lo;
        uint32_t bans = 0;
        order.resize(cnt);
        std::iota(order.begin(), order.end(), lo);
        for (uint32_t e = lo; e < lo + cnt; ++e) {
            WRK_ARG(ctx, ids[e] < V, "set %u: id %u >= vocab %u", s, ids[e], V);
            WRK_ARG(ctx, values[e] == values[e] && values[e] != INFINITY, "set %u: the bias of token %u is NaN or +inf", s, ids[e]);
            bans += values[e] == -INFINITY;
        }
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return ids[a] < ids[b]; });
        for (uint32_t k = 0; k < cnt; ++k) {
            WRK_ARG(ctx, k == 0 || ids[order[k]] != ids[order[k - 1]], "set %u: token %u twice", s, ids[order[k]]);
            sid.push_back(ids[order[k]]);
            sval.push_back(values[order[k]]);
        }
        WRK_ARG(ctx, bans < V, "set %u bans every token", s);
    }
    const uint32_t E = set_offsets[S];
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_layout lay;
    const size_t o_off = lay.add((size_t)(S + 1) * 4), o_ids = lay.add((size_t)E * 4 + 4), o_val = lay.add((size_t)E * 4 + 4);
    wrk_logit_bias* lb = new wrk_logit_bias;       // before the device allocation: a throw leaves nothing behind
    lb->ctx = ctx;
    lb->num_vocab = V; lb->num_sets = S; lb->num_entries = E;
    if (hipMalloc(&lb->mem, lay.total) != hipSuccess) {
        delete lb;
        return wrk_fail(ctx, WRK_E_OOM, "hipMalloc of %zu bytes for a logit bias", lay.total);
    }
    lb->offsets = (uint32_t*)((char*)lb->mem + o_off);
    lb->ids = (uint32_t*)((char*)lb->mem + o_ids);
    lb->values = (float*)((char*)lb->mem + o_val);
    int32_t rc = wrk_buf_write_raw(ctx, lb->offsets, set_offsets, (size_t)(S + 1) * 4);
    if (rc == WRK_OK && E) rc = wrk_buf_write_raw(ctx, lb->ids, sid.data(), (size_t)E * 4);
    if (rc == WRK_OK && E) rc = wrk_buf_write_raw(ctx, lb->values, sval.data(), (size_t)E * 4);
    if (rc == WRK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = wrk_fail(ctx, WRK_E_HIP, "logit bias upload failed");
    if (rc != WRK_OK) { wrk_logit_bias_destroy(lb); return rc; }
    *out = lb;
    return WRK_OK;
}

int32_t wrk_logit_bias_destroy(wrk_logit_bias* lb) {
    if (!lb) return WRK_E_ARG;
    {
        std::lock_guard<std::recursive_mutex> lk(lb->ctx->mu);
        hipSetDevice(lb->ctx->device);
        hipStreamSynchronize(lb->ctx->stream);      // no step in flight still reads the sets
        hipFree(lb->mem);
    }
    delete lb;
    return WRK_OK;
}

// the blocking launch both entry points below share: rows of `in` biased into `out` (the same rows: in place)
static int32_t bias_rows_blocking(wrk_ctx* ctx, const float* in, uint32_t in_stride, float* out, uint32_t out_stride, uint32_t V, uint32_t n,
                                  const wrk_logit_bias* lb, const uint32_t* sets) {
    std::vector<uint32_t> st;
    WRK_ARG(ctx, n == 0 || sets, "sets required");
    const int32_t rc = wrk_bias_pack(ctx, lb, sets, n, V, st);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::BiasParam)), o_st = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    const wrk::BiasParam par = lb->param(dev.at<uint32_t>(o_st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_st), st.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::bias_rows(ctx->stream, in, V, in_stride, n, dev.at<wrk::BiasParam>(o_par), out, out_stride);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_bias_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const wrk_logit_bias* lb, const uint32_t* sets) {
    if (!ctx || !logits || !lb) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_bias_logits", wrk::SAMPLE_MAX_VOCAB);
    if (rc != WRK_OK) return rc;
    return bias_rows_blocking(ctx, (const float*)logits->ptr, stride, (float*)logits->ptr, stride, V, n, lb, sets);
}

// Not part of the ABI (include/wrk_hip.h does not declare it): the copying launch of a step program -- rows of `in` biased into the
// rows of another buffer `out`, each with its own stride, `in` left as it is -- for tests/test_gpu_bias.py, which the decode loops
// reach only at the vocabulary of the test models.  Blocking
int32_t wrk_bias_rows_copy(wrk_ctx* ctx, const wrk_buf* in, uint32_t in_stride, wrk_buf* out, uint32_t out_stride, uint32_t V, uint32_t n,
                           const wrk_logit_bias* lb, const uint32_t* sets) {
    if (!ctx || !in || !out || !lb) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = wrk_rows_check(ctx, in, V, in_stride, n, "wrk_bias_rows_copy", wrk::SAMPLE_MAX_VOCAB);
    if (rc == WRK_OK) rc = wrk_rows_check(ctx, out, V, out_stride, n, "wrk_bias_rows_copy", wrk::SAMPLE_MAX_VOCAB);
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, in != out && in->ptr != out->ptr, "wrk_bias_rows_copy: in and out are one buffer");
    return bias_rows_blocking(ctx, (const float*)in->ptr, in_stride, (float*)out->ptr, out_stride, V, n, lb, sets);
}

}  // extern "C"
