// Repetition penalties on the device for gfx950 (ChatRWKV's PIPELINE.generate: alpha_presence, alpha_frequency, alpha_decay,
// token_ban).  An occurrence table (wrk_occurrence) holds, per state slot, count[n] (f32) and flags[n] (u8: bit 0 present, bit 1
// banned), and one weight vector w[n] for all slots.  Per row x of a sequence with (presence ap, frequency af, decay g):
//   x'[n] = -inf                          if banned[n]
//         = x[n] - (ap + count[n] * af)   if present[n]      (t = count * af; t = ap + t; x - t: three f32 roundings, no FMA)
//         = x[n]                          otherwise
// and after the draw of y:  count[n] *= g for every n; then count[y] += w[y]; then present[y] = 1.  See DESIGN.md §7c.
//
// Both kernels cover a row with ceil(V / 1024) workgroups of 256 threads (grid (slices, rows)), 4 elements per thread, so that one
// 65 536-token row spreads over 64 workgroups instead of one CU.  The update has no atomics: the thread that owns element y also does
// its decay, so the result is the same on every replay.  Rows with g == 1 touch only element y.
#include "wrk_rows_dev.h"
#include "wrk_runner.h" // wrk_buf_write_raw

#include <cmath>

namespace wrk {

static constexpr uint32_t PEN_THREADS = 256;
static constexpr uint32_t PEN_TILE = PEN_THREADS * 4;      // elements per workgroup

__device__ __forceinline__ float penalize_one(float x, float c, uint32_t f, float ap, float af) {
    if (f & 2u) return -INFINITY;
    if (f & 1u) {
        float t = c * af;
        t = ap + t;
        return x - t;
    }
    return x;
}

// VEC: every row of src / dst / count starts 16-byte aligned and v % 4 == 0, so thread tid owns the float4 at a + 4 * tid; otherwise
// it owns a + tid + 256 * j (j < 4), one coalesced scalar access each.  src and dst may be the same rows (in place).
template <bool VEC>
__global__ void __launch_bounds__(PEN_THREADS) penalize_rows_kernel(const float* src, uint32_t v, uint32_t src_stride,
                                                                    const PenaltyParam* __restrict__ par, float* dst, uint32_t dst_stride) {
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const PenaltyParam p = par[r];
    const float* x = src + (size_t)r * src_stride;
    float* y = dst + (size_t)r * dst_stride;
    const uint32_t a = blockIdx.x * PEN_TILE;
    if (VEC) {
        const uint32_t i = a + tid * 4;
        if (i >= v) return;
        const f32x4 xv = *(const f32x4*)(x + i);
        const f32x4 cv = *(const f32x4*)(p.count + i);
        const uint32_t fv = *(const uint32_t*)(p.flags + i);
        f32x4 o;
        o.x = penalize_one(xv.x, cv.x, fv & 0xffu, p.presence, p.frequency);
        o.y = penalize_one(xv.y, cv.y, (fv >> 8) & 0xffu, p.presence, p.frequency);
        o.z = penalize_one(xv.z, cv.z, (fv >> 16) & 0xffu, p.presence, p.frequency);
        o.w = penalize_one(xv.w, cv.w, fv >> 24, p.presence, p.frequency);
        *(f32x4*)(y + i) = o;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = a + j * PEN_THREADS + tid;
            if (i < v) y[i] = penalize_one(x[i], p.count[i], p.flags[i], p.presence, p.frequency);
        }
    }
}

// row r applies the ntok tokens tokens[r * ntok ..] in order.  g != 1: every thread decays its own 4 elements once per token and adds
// the weight of each token it owns right after that token's decay; g == 1: thread 0 of the workgroup that owns a token adds its weight
// (in list order, so repeats add one after another) and nothing else is read or written
template <bool VEC>
__device__ __forceinline__ void occurrence_update_row(uint32_t v, const PenaltyParam* __restrict__ par, const uint32_t* __restrict__ tokens,
                                                      uint32_t ntok) {
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const PenaltyParam p = par[r];
    const uint32_t* tk = tokens + (size_t)r * ntok;
    const uint32_t a = blockIdx.x * PEN_TILE;
    const uint32_t end = a + PEN_TILE < v ? a + PEN_TILE : v;
    if (p.decay == 1.0f) {
        if (tid != 0) return;
        for (uint32_t k = 0; k < ntok; ++k) {
            const uint32_t t = tk[k];
            if (t >= a && t < end) {
                p.count[t] = p.count[t] + p.weight[t];
                p.flags[t] |= 1u;
            }
        }
        return;
    }
    uint32_t idx[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) idx[j] = VEC ? a + tid * 4 + j : a + j * PEN_THREADS + tid;
    float c[4];
    if (VEC) {
        if (idx[0] >= v) return;
        const f32x4 cv = *(const f32x4*)(p.count + idx[0]);
        c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) c[j] = idx[j] < v ? p.count[idx[j]] : 0.0f;
    }
    uint32_t hit = 0;       // bit j: element idx[j] was drawn
    for (uint32_t k = 0; k < ntok; ++k) {
        const uint32_t t = tk[k];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            c[j] = c[j] * p.decay;
            if (t == idx[j]) { c[j] = c[j] + p.weight[t]; hit |= 1u << j; }
        }
    }
    if (VEC) {
        *(f32x4*)(p.count + idx[0]) = f32x4{c[0], c[1], c[2], c[3]};
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (idx[j] < v) p.count[idx[j]] = c[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (hit & (1u << j)) p.flags[idx[j]] |= 1u;
}

// a row whose draw does not count returns before it reads anything else of its row
template <bool VEC>
__global__ void __launch_bounds__(PEN_THREADS) occurrence_update_kernel(uint32_t v, const PenaltyParam* __restrict__ par,
                                                                        const uint32_t* __restrict__ tokens, uint32_t ntok, const RowGate gate) {
    if (!row_counts(gate, blockIdx.y)) return;
    occurrence_update_row<VEC>(v, par, tokens, ntok);
}

// rows of an occurrence table start at slot * v: 16-byte aligned counts (and 4-byte aligned flags) exactly when v % 4 == 0
static bool pen_vec(uint32_t v) { return v % 4 == 0; }

void penalize_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, const PenaltyParam* par, float* dst,
                   uint32_t dst_stride) {
    if (n == 0 || v == 0) return;
    const dim3 grid((v + PEN_TILE - 1) / PEN_TILE, n);
    if (pen_vec(v) && src_stride % 4 == 0 && dst_stride % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0)
        penalize_rows_kernel<true><<<grid, PEN_THREADS, 0, s>>>(src, v, src_stride, par, dst, dst_stride);
    else penalize_rows_kernel<false><<<grid, PEN_THREADS, 0, s>>>(src, v, src_stride, par, dst, dst_stride);
}

void occurrence_update(hipStream_t s, uint32_t v, uint32_t n, const PenaltyParam* par, const uint32_t* tokens, uint32_t ntok, const RowGate& gate) {
    if (n == 0 || v == 0 || ntok == 0) return;
    const dim3 grid((v + PEN_TILE - 1) / PEN_TILE, n);
    if (pen_vec(v)) occurrence_update_kernel<true><<<grid, PEN_THREADS, 0, s>>>(v, par, tokens, ntok, gate);
    else occurrence_update_kernel<false><<<grid, PEN_THREADS, 0, s>>>(v, par, tokens, ntok, gate);
}

}  // namespace wrk

wrk::PenaltyParam wrk_occurrence::row(uint32_t slot, float presence, float frequency, float decay) const {
    return wrk::PenaltyParam{counts + (size_t)slot * num_vocab, flags + (size_t)slot * num_vocab, weights, presence, frequency, decay, 0u};
}

int32_t wrk_penalty_pack(wrk_ctx* ctx, const wrk_occurrence* occ, uint32_t first, uint32_t n, uint32_t V, const float* presence,
                         const float* frequency, const float* decay, std::vector<wrk::PenaltyParam>& out) {
    WRK_ARG(ctx, occ, "occurrence table required");
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    WRK_ARG(ctx, presence && frequency, "presence and frequency arrays are required");
    WRK_ARG(ctx, occ->num_vocab == V, "occurrence table of %u tokens, logits of %u", occ->num_vocab, V);
    WRK_ARG(ctx, (uint64_t)first + n <= occ->num_batch, "slots [%u, %u) exceed the table's %u", first, first + n, occ->num_batch);
    out.resize(n);
    for (uint32_t b = 0; b < n; ++b) {
        const float ap = presence[b], af = frequency[b], g = decay ? decay[b] : 1.0f;
        WRK_ARG(ctx, finite_f32(ap), "presence[%u] = %g: must be finite", b, (double)ap);
        WRK_ARG(ctx, finite_f32(af), "frequency[%u] = %g: must be finite", b, (double)af);
        WRK_ARG(ctx, g >= 0.0f && g <= 1.0f, "decay[%u] = %g: must be in [0, 1]", b, (double)g);
        out[b] = occ->row(first + b, ap, af, g);
    }
    return WRK_OK;
}

extern "C" {

int32_t wrk_occurrence_create(wrk_ctx* ctx, uint32_t B, uint32_t V, wrk_occurrence** out) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, B >= 1 && B <= 65535, "num_batch %u: must be in [1, 65535]", B);
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)B * V;
    wrk_dev_layout lay;
    const size_t o_c = lay.add(n * 4), o_w = lay.add((size_t)V * 4), o_f = lay.add(n);
    void* mem = nullptr;
    WRK_HIP(ctx, hipMalloc(&mem, lay.total));
    wrk_occurrence* occ = new wrk_occurrence;
    occ->ctx = ctx;
    occ->num_batch = B;
    occ->num_vocab = V;
    occ->mem = mem;
    occ->counts = (float*)((char*)mem + o_c);
    occ->weights = (float*)((char*)mem + o_w);
    occ->flags = (uint8_t*)((char*)mem + o_f);
    hipError_t e = hipMemsetAsync(occ->counts, 0, n * 4, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(occ->flags, 0, n, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    int32_t rc = e == hipSuccess ? wrk_occurrence_set_weights(ctx, occ, nullptr)
                                 : wrk_fail(ctx, WRK_E_HIP, "occurrence table: %s", hipGetErrorString(e));
    if (rc != WRK_OK) { wrk_occurrence_destroy(occ); return rc; }
    *out = occ;
    return WRK_OK;
}

int32_t wrk_occurrence_destroy(wrk_occurrence* occ) {
    if (!occ) return WRK_E_ARG;
    {
        std::lock_guard<std::recursive_mutex> lk(occ->ctx->mu);
        hipSetDevice(occ->ctx->device);
        hipStreamSynchronize(occ->ctx->stream);     // no step in flight still reads the table
        hipFree(occ->mem);
    }
    delete occ;
    return WRK_OK;
}

int32_t wrk_occurrence_set_weights(wrk_ctx* ctx, wrk_occurrence* occ, const float* weights) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    std::vector<float> w(occ->num_vocab, 1.0f);
    if (weights)
        for (uint32_t i = 0; i < occ->num_vocab; ++i) {
            WRK_ARG(ctx, finite_f32(weights[i]) && weights[i] >= 0.0f, "weights[%u] = %g: must be finite and >= 0", i, (double)weights[i]);
            w[i] = weights[i];
        }
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    return wrk_buf_write_raw(ctx, occ->weights, w.data(), w.size() * 4);
}

int32_t wrk_occurrence_ban(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t b, const uint32_t* tokens, uint32_t n, int32_t banned) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    WRK_ARG(ctx, b < occ->num_batch, "slot %u >= %u", b, occ->num_batch);
    WRK_ARG(ctx, n == 0 || tokens, "tokens required");
    const uint32_t V = occ->num_vocab;
    for (uint32_t i = 0; i < n; ++i) WRK_ARG(ctx, tokens[i] < V, "token %u: id %u >= vocab %u", i, tokens[i], V);
    if (n == 0) return WRK_OK;
    // read-modify-write of the slot's flags: the ban count is recomputed from the row itself, so it cannot drift from the device
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> f(V);
    uint8_t* row = occ->flags + (size_t)b * V;
    WRK_HIP(ctx, hipMemcpyAsync(f.data(), row, V, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n; ++i) f[tokens[i]] = banned ? (f[tokens[i]] | 2u) : (f[tokens[i]] & ~2u);
    uint32_t nb = 0;
    for (uint32_t i = 0; i < V; ++i) nb += (f[i] >> 1) & 1u;
    WRK_ARG(ctx, nb < V, "the ban would leave slot %u with no allowed token", b);
    return wrk_buf_write_raw(ctx, row, f.data(), V);
}

int32_t wrk_occurrence_add(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t b, const uint32_t* tokens, uint32_t n, float decay) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_occurrence_add is blocking: not inside a capture");
    WRK_ARG(ctx, n == 0 || tokens, "tokens required");
    const uint32_t V = occ->num_vocab;
    for (uint32_t i = 0; i < n; ++i) WRK_ARG(ctx, tokens[i] < V, "token %u: id %u >= vocab %u", i, tokens[i], V);
    WRK_ARG(ctx, b < occ->num_batch, "slot %u >= %u", b, occ->num_batch);
    const float zero = 0.0f;
    std::vector<wrk::PenaltyParam> par;
    const int32_t rc = wrk_penalty_pack(ctx, occ, b, 1, V, &zero, &zero, &decay, par);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::PenaltyParam)), o_tok = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), par.data(), sizeof(wrk::PenaltyParam), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tok), tokens, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::occurrence_update(ctx->stream, V, 1, dev.at<wrk::PenaltyParam>(o_par), dev.at<uint32_t>(o_tok), n, wrk::RowGate{});
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_occurrence_back(wrk_ctx* ctx, const wrk_occurrence* occ, uint32_t b, float* counts, uint32_t* flags) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    WRK_ARG(ctx, b < occ->num_batch, "slot %u >= %u", b, occ->num_batch);
    WRK_ARG(ctx, counts && flags, "counts and flags are required");
    const uint32_t V = occ->num_vocab;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> f(V);
    WRK_HIP(ctx, hipMemcpyAsync(counts, occ->counts + (size_t)b * V, (size_t)V * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(f.data(), occ->flags + (size_t)b * V, V, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < V; ++i) flags[i] = f[i];
    return WRK_OK;
}

int32_t wrk_occurrence_load(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t b, const float* counts, const uint32_t* flags) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    WRK_ARG(ctx, b < occ->num_batch, "slot %u >= %u", b, occ->num_batch);
    WRK_ARG(ctx, (counts == nullptr) == (flags == nullptr), "counts and flags: both, or neither (reset)");
    const uint32_t V = occ->num_vocab;
    std::vector<float> c(V, 0.0f);
    std::vector<uint8_t> f(V, 0);
    if (counts) {
        uint32_t nb = 0;
        for (uint32_t i = 0; i < V; ++i) {
            WRK_ARG(ctx, finite_f32(counts[i]), "counts[%u] = %g: must be finite", i, (double)counts[i]);
            WRK_ARG(ctx, flags[i] <= 3u, "flags[%u] = %u: only bits 0 (present) and 1 (banned)", i, flags[i]);
            c[i] = counts[i];
            f[i] = (uint8_t)flags[i];
            nb += flags[i] >> 1;
        }
        WRK_ARG(ctx, nb < V, "the flags ban every token of slot %u", b);
    }
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    int32_t rc = wrk_buf_write_raw(ctx, occ->counts + (size_t)b * V, c.data(), (size_t)V * 4);
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, occ->flags + (size_t)b * V, f.data(), V);
    return rc;
}

int32_t wrk_penalize_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const wrk_occurrence* occ,
                            uint32_t first, const float* presence, const float* frequency) {
    if (!ctx || !logits || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_penalize_logits", 0);
    std::vector<wrk::PenaltyParam> par;
    if (rc == WRK_OK) rc = wrk_penalty_pack(ctx, occ, first, n, V, presence, frequency, nullptr, par);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    dev.add((size_t)n * sizeof(wrk::PenaltyParam));
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.base, par.data(), (size_t)n * sizeof(wrk::PenaltyParam), hipMemcpyHostToDevice, ctx->stream));
    wrk::penalize_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, dev.at<wrk::PenaltyParam>(0), (float*)logits->ptr, stride);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

}  // extern "C"
