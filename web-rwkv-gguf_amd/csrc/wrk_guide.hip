// Classifier-free guidance on the device for gfx950: the guided row of a conditional and an unconditional logits row (Hugging Face's
// guidance_scale with negative_prompt_ids, llama.cpp's --cfg-scale with --cfg-negative-prompt, text-generation-webui's negative
// prompt).  See DESIGN.md §7r.
//
// The rows are mixed raw, without a log-softmax: log-softmaxed rows differ from the raw ones by one constant per row, and the mix of two
// such rows differs from the mix of the raw rows by one constant per row again, which no link of the pick chain sees.  So one
// element-wise pass makes the guided row.  With c = row_norm(xc), u = row_norm(xu) and the row's scale s, the first case that applies:
//   s == 1      the bits of xc (the row is off: NaN payloads and -0 included)
//   c == -inf   -inf            impossible under the prompt stays impossible
//   c == +inf   +inf
//   u == -inf   c
//   s == 0      u
//   u == +inf   -inf if s > 1, else +inf
//   else        d = c - u, p = s * d, out = p + u: three IEEE f32 operations, never contracted; an overflow of d or p to +-inf is the
//               result, the limit of the expression
// Outside s == 1 rows the result is never NaN.
//
//   guide_rows    grid (spans of GUIDE_SPAN tokens, rows): out row r from in rows r (conditional) and n + r (unconditional) and the
//                 scale par[r], which is device data: one captured program serves any scales.  16-byte loads and stores when the bases
//                 and the strides allow, one coalesced scalar access per element otherwise; nothing outside [0, v) of a row is written
//   guide_follow  argmax[n + r] = argmax[r]: the partner sequences of a guided step are fed the tokens of the conditional ones
//
// Plain vector loads and stores only; no kernel waits on another.
#include "wrk_rows_dev.h"
#include "wrk_runner.h"

namespace wrk {

static constexpr uint32_t GUIDE_THREADS = 256;
static constexpr uint32_t GUIDE_TILE = GUIDE_THREADS * 4;           // tokens of one tile: 4 per thread
static constexpr uint32_t GUIDE_TILES = 4;                          // tiles per workgroup
static constexpr uint32_t GUIDE_SPAN = GUIDE_TILE * GUIDE_TILES;    // tokens per workgroup

// the contract's cases below s == 1, which the caller has taken; the intrinsics keep the three roundings under any -ffp-contract
__device__ __forceinline__ uint32_t guide_mix(uint32_t xc, uint32_t xu, float s) {
    const float c = row_norm(__uint_as_float(xc)), u = row_norm(__uint_as_float(xu));
    float o;
    if (c == -INFINITY || c == INFINITY) o = c;
    else if (u == -INFINITY) o = c;
    else if (s == 0.0f) o = u;
    else if (u == INFINITY) o = s > 1.0f ? -INFINITY : INFINITY;
    else o = __fadd_rn(__fmul_rn(s, __fsub_rn(c, u)), u);
    return __float_as_uint(o);
}

// VEC: every row of in / out starts 16-byte aligned and v % 4 == 0, so thread tid owns the 4 tokens at a + 4 * tid of each tile; otherwise
// it owns a + tid + 256 * j (j < 4), one coalesced scalar access each.  A row with s == 1 moves its logits as u32: no float operation
// touches them
template <bool VEC>
__global__ void __launch_bounds__(GUIDE_THREADS) guide_rows_kernel(const uint32_t* in, uint32_t v, uint32_t in_stride, uint32_t n,
                                                                   const float* __restrict__ par, uint32_t* out, uint32_t out_stride) {
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const uint32_t* xc = in + (size_t)r * in_stride;
    const uint32_t* xu = in + (size_t)(n + r) * in_stride;
    uint32_t* y = out + (size_t)r * out_stride;
    const uint32_t a0 = blockIdx.x * GUIDE_SPAN;
    const float s = par[r];
    const bool off = s == 1.0f;
    if (VEC) {
        u32x4 cv[GUIDE_TILES], uv[GUIDE_TILES];
#pragma unroll
        for (uint32_t k = 0; k < GUIDE_TILES; ++k) {
            const uint32_t i = a0 + k * GUIDE_TILE + tid * 4;
            if (i < v) {
                cv[k] = *(const u32x4*)(xc + i);
                if (!off) uv[k] = *(const u32x4*)(xu + i);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < GUIDE_TILES; ++k) {
            const uint32_t i = a0 + k * GUIDE_TILE + tid * 4;
            if (i < v) {
                u32x4 o = cv[k];
                if (!off) {
                    o.x = guide_mix(cv[k].x, uv[k].x, s); o.y = guide_mix(cv[k].y, uv[k].y, s);
                    o.z = guide_mix(cv[k].z, uv[k].z, s); o.w = guide_mix(cv[k].w, uv[k].w, s);
                }
                *(u32x4*)(y + i) = o;
            }
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < GUIDE_TILES; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = a0 + k * GUIDE_TILE + j * GUIDE_THREADS + tid;
                if (i < v) y[i] = off ? xc[i] : guide_mix(xc[i], xu[i], s);
            }
    }
}

void guide_rows(hipStream_t s, const float* in, uint32_t v, uint32_t in_stride, uint32_t n, const float* par, float* out, uint32_t out_stride) {
    if (n == 0 || v == 0) return;
    const dim3 grid((v + GUIDE_SPAN - 1) / GUIDE_SPAN, n);
    const uint32_t* src = (const uint32_t*)in;
    uint32_t* dst = (uint32_t*)out;
    if (v % 4 == 0 && in_stride % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0)
        guide_rows_kernel<true><<<grid, GUIDE_THREADS, 0, s>>>(src, v, in_stride, n, par, dst, out_stride);
    else guide_rows_kernel<false><<<grid, GUIDE_THREADS, 0, s>>>(src, v, in_stride, n, par, dst, out_stride);
}

__global__ void guide_follow_kernel(uint32_t* argmax, uint32_t n) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) argmax[n + r] = argmax[r];
}

void guide_follow(hipStream_t s, uint32_t* argmax, uint32_t n) {
    if (n == 0) return;
    guide_follow_kernel<<<(n + 63) / 64, 64, 0, s>>>(argmax, n);
}

}  // namespace wrk

int32_t wrk_guide_pack(wrk_ctx* ctx, const float* scale, uint32_t n, uint32_t V, std::vector<float>& out) {
    WRK_ARG(ctx, n == 0 || scale, "guidance_scale required");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "guidance: vocabulary of %u tokens", V);
    out.assign(n, 1.0f);
    for (uint32_t r = 0; r < n; ++r) {
        WRK_ARG(ctx, finite_f32(scale[r]) && scale[r] >= 0.0f, "guidance_scale[%u] = %g: must be finite and >= 0", r, (double)scale[r]);
        out[r] = scale[r];
    }
    return WRK_OK;
}

extern "C" {

int32_t wrk_guide_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const float* scale, wrk_buf* out,
                         uint32_t out_stride) {
    if (!ctx || !logits || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, n <= 0x7fffffffu, "num_rows %u", n);
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, 2 * n, "wrk_guide_logits", wrk::SAMPLE_MAX_VOCAB);
    if (rc == WRK_OK) rc = wrk_rows_check(ctx, out, V, out_stride, n, "wrk_guide_logits", wrk::SAMPLE_MAX_VOCAB);
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, logits != out && logits->ptr != out->ptr, "wrk_guide_logits: logits and out are one buffer");
    std::vector<float> sc;
    rc = wrk_guide_pack(ctx, scale, n, V, sc);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_sc = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_sc), sc.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::guide_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, dev.at<float>(o_sc), (float*)out->ptr, out_stride);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

}  // extern "C"
