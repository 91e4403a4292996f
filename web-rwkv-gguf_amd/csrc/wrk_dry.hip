// DRY ("don't repeat yourself") and the no-repeat-n-gram ban on the device for gfx950: penalties that look at the ORDER of what a sequence
// generated (text-generation-webui / koboldcpp / llama.cpp's dry_*, Hugging Face's no_repeat_ngram_size).  See DESIGN.md §7n.
//
// A token window (wrk_token_window) holds, per state slot, the last `cap` tokens that counted as a ring: ring[cap] and meta = (length,
// next write position).  A row with window w[0..n), last = w[n-1] and the call's breaker set Bk has, for every i in [0, n-2] with
// w[i] == last and t = w[i+1] not in Bk, the match length m = 1 + #{consecutive k >= 1 : w[i-k] == w[n-1-k], w[n-1-k] not in Bk},
// capped at WRK_DRY_MAX_MATCH, and M[t] = the max over i; nothing matches when n < 2 or last is in Bk.  Then
//   x'[t] = -inf            if no_repeat != 0 and M[t] >= no_repeat - 1
//         = x[t] - pen[M]   else if multiplier != 0 and M[t] >= allowed        (one f32 subtraction, pen computed on the host)
//         = x[t]            otherwise: no instruction touches the element
//
//   dry_rows      one workgroup of 256 threads per row.  The ring is unwrapped into LDS (at most 16 KB); wave 0 finds, with one ballot,
//                 the length at which the tail side alone stops every match (the cap, the start of the window, a breaker at w[n-1-m]),
//                 so the compare loop of a candidate tests one LDS word against one broadcast LDS word per step, at most 49 steps.
//                 Candidates are strided over the threads.  M[t] is combined through the row's u32 scratch [V], zero between launches:
//                 atomicMax(scratch[t], m); barrier; every candidate exchanges scratch[t] with 0 and the one that receives a non-zero
//                 M changes x[t].  Integer max is order-free, so the result does not depend on the thread order, every touched token is
//                 changed exactly once, and the scratch is clean again when the kernel ends
//   copy_rows     grid (ceil(V / 1024), rows): the head output into the rows dry_rows works on, moved as bits
//   window_push   one row per thread, under the step's RowGate: a row whose draw does not count keeps its window
//
// Plain vector loads and stores and ordinary vector atomics only; no kernel waits on a flag, the host or another workgroup.
#include "wrk_rows_dev.h"
#include "wrk_runner.h" // wrk_buf_write_raw

#include <cfloat>

namespace wrk {

static constexpr uint32_t DRY_THREADS = 256;
static constexpr uint32_t DRY_COPY_TILE = DRY_THREADS * 4;
static constexpr uint32_t DRY_NEG_INF_BITS = 0xFF800000u;

__global__ void __launch_bounds__(DRY_THREADS) dry_rows_kernel(float* x, uint32_t v, uint32_t stride, const DryParam* __restrict__ par,
                                                               const DryBreakers* __restrict__ brk, uint32_t* scratch) {
    __shared__ uint32_t w[WRK_MAX_TOKEN_WINDOW];
    __shared__ uint32_t bk[WRK_MAX_DRY_BREAKERS];
    __shared__ uint32_t tail_stop;
    const uint32_t r = blockIdx.x, tid = threadIdx.x;
    const DryParam* p = par + r;
    const float mult = p->multiplier;
    const uint32_t no_repeat = p->no_repeat, allowed = p->allowed;
    if (mult == 0.0f && no_repeat == 0u) return;           // an all-off row: nothing of it is read or written
    const uint32_t cap = p->cap < WRK_MAX_TOKEN_WINDOW ? p->cap : WRK_MAX_TOKEN_WINDOW;
    uint32_t n = p->meta[0], pos = p->meta[1];
    if (n > cap) n = cap;
    if (n < 2u) return;
    if (pos >= cap) pos = 0;
    const uint32_t nb = brk->count < WRK_MAX_DRY_BREAKERS ? brk->count : WRK_MAX_DRY_BREAKERS;
    // logical order, oldest first: the oldest token sits n places behind the write position
    const uint32_t start = pos >= n ? pos - n : pos + cap - n;
    for (uint32_t j = tid; j < n; j += DRY_THREADS) {
        const uint32_t k = start + j;
        w[j] = p->ring[k >= cap ? k - cap : k];
    }
    if (tid < nb) bk[tid] = brk->ids[tid];
    __syncthreads();
    auto is_breaker = [&](uint32_t t) {
        bool hit = false;
        for (uint32_t k = 0; k < nb; ++k) hit |= bk[k] == t;
        return hit;
    };
    // lane m of wave 0: does the tail side stop a match at length m?  (lane 0: is `last` a breaker, which stops everything)
    if (tid < WAVE) {
        bool stop;
        if (tid == 0) stop = is_breaker(w[n - 1]);
        else if (tid >= WRK_DRY_MAX_MATCH || tid > n - 1) stop = true;
        else stop = is_breaker(w[n - 1 - tid]);
        const unsigned long long b = __ballot(stop);
        // bit 0: no match at all; else the lowest set bit in [1, WRK_DRY_MAX_MATCH] is the longest length any candidate can reach
        if (tid == 0) tail_stop = (b & 1ull) ? 0u : (uint32_t)__ffsll((long long)(b & ~1ull)) - 1u;
    }
    __syncthreads();
    const uint32_t mcap = tail_stop;
    if (mcap == 0u) return;
    const uint32_t last = w[n - 1];
    uint32_t* scr = scratch + (size_t)r * v;
    for (uint32_t i = tid; i + 1 < n; i += DRY_THREADS) {
        if (w[i] != last) continue;
        const uint32_t t = w[i + 1];
        if (t >= v || is_breaker(t)) continue;
        uint32_t m = 1;
        while (m < mcap && i >= m && w[i - m] == w[n - 1 - m]) ++m;       // w[n - 1 - m]: one address for the whole wave
        atomicMax(scr + t, m);
    }
    // every atomicMax of the workgroup has reached memory before any exchange below is issued
    __threadfence();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float* xr = x + (size_t)r * stride;
    for (uint32_t i = tid; i + 1 < n; i += DRY_THREADS) {
        if (w[i] != last) continue;
        const uint32_t t = w[i + 1];
        if (t >= v || is_breaker(t)) continue;
        const uint32_t M = atomicExch(scr + t, 0u);
        if (M == 0u) continue;                              // another candidate of the same token took it
        if (no_repeat != 0u && M >= no_repeat - 1u) ((uint32_t*)xr)[t] = DRY_NEG_INF_BITS;
        else if (mult != 0.0f && M >= allowed) xr[t] = xr[t] - p->pen[M];
    }
}

// VEC: every row of src / dst starts 16-byte aligned and v % 4 == 0, so thread tid owns the 4 elements at a + 4 * tid; otherwise it owns
// a + tid + 256 * j (j < 4), one coalesced scalar access each.  Logits move as u32: no float operation touches them
template <bool VEC>
__global__ void __launch_bounds__(DRY_THREADS) copy_rows_kernel(const uint32_t* __restrict__ src, uint32_t v, uint32_t src_stride,
                                                                uint32_t* __restrict__ dst, uint32_t dst_stride) {
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const uint32_t* x = src + (size_t)r * src_stride;
    uint32_t* y = dst + (size_t)r * dst_stride;
    const uint32_t a = blockIdx.x * DRY_COPY_TILE;
    if (VEC) {
        const uint32_t i = a + tid * 4;
        if (i < v) *(u32x4*)(y + i) = *(const u32x4*)(x + i);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = a + j * DRY_THREADS + tid;
            if (i < v) y[i] = x[i];
        }
    }
}

// a row whose draw does not count returns before it reads anything else of its row; a token outside the vocabulary (none reaches here:
// the picks return ids < v) is not stored
__global__ void __launch_bounds__(DRY_THREADS) window_push_kernel(uint32_t v, uint32_t n, const DryParam* __restrict__ par,
                                                                  const uint32_t* __restrict__ tokens, const RowGate gate) {
    const uint32_t r = blockIdx.x * DRY_THREADS + threadIdx.x;
    if (r >= n || !row_counts(gate, r)) return;
    const uint32_t t = tokens[r];
    if (t >= v) return;
    const DryParam* p = par + r;
    const uint32_t cap = p->cap;
    if (cap == 0u) return;
    uint32_t len = p->meta[0], pos = p->meta[1];
    if (pos >= cap) pos = 0;
    p->ring[pos] = t;
    p->meta[0] = len < cap ? len + 1 : cap;
    p->meta[1] = pos + 1 == cap ? 0u : pos + 1;
}

void dry_rows(hipStream_t s, float* x, uint32_t v, uint32_t stride, uint32_t n, const DryParam* par, const DryBreakers* brk, uint32_t* scratch) {
    if (n == 0 || v == 0) return;
    dry_rows_kernel<<<n, DRY_THREADS, 0, s>>>(x, v, stride, par, brk, scratch);
}

void copy_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, float* dst, uint32_t dst_stride) {
    if (n == 0 || v == 0) return;
    const dim3 grid((v + DRY_COPY_TILE - 1) / DRY_COPY_TILE, n);
    if (v % 4 == 0 && src_stride % 4 == 0 && dst_stride % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0)
        copy_rows_kernel<true><<<grid, DRY_THREADS, 0, s>>>((const uint32_t*)src, v, src_stride, (uint32_t*)dst, dst_stride);
    else copy_rows_kernel<false><<<grid, DRY_THREADS, 0, s>>>((const uint32_t*)src, v, src_stride, (uint32_t*)dst, dst_stride);
}

void window_push(hipStream_t s, uint32_t v, uint32_t n, const DryParam* par, const uint32_t* tokens, const RowGate& gate) {
    if (n == 0 || v == 0) return;
    window_push_kernel<<<(n + DRY_THREADS - 1) / DRY_THREADS, DRY_THREADS, 0, s>>>(v, n, par, tokens, gate);
}

}  // namespace wrk

// pen[m] of a row: 0 below allowed_length, else multiplier * base^(m - allowed_length) as repeated f64 products, rounded to f32 and
// clamped to FLT_MAX -- the same table on every IEEE host
static void dry_penalty_table(float multiplier, float base, uint32_t allowed, float* pen) {
    for (uint32_t m = 0; m < WRK_DRY_MAX_MATCH + 2; ++m) pen[m] = 0.0f;
    double p = (double)multiplier;
    for (uint32_t m = allowed; m <= WRK_DRY_MAX_MATCH; ++m) {
        pen[m] = p >= (double)FLT_MAX ? FLT_MAX : (float)p;
        p = p * (double)base;
    }
}

int32_t wrk_dry_pack(wrk_ctx* ctx, const wrk_dry_args& a, uint32_t first, uint32_t n, uint32_t slots, uint32_t V, std::vector<wrk::DryParam>& rows,
                     wrk::DryBreakers& brk) {
    const wrk_token_window* win = a.window;
    WRK_ARG(ctx, win, "token window required");
    WRK_ARG(ctx, win->ctx == ctx, "the token window belongs to another context");
    WRK_ARG(ctx, win->num_vocab == V, "token window of %u tokens, logits of %u", win->num_vocab, V);
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "DRY: vocabulary of %u tokens", V);
    const uint32_t own = n < slots ? n : slots;
    WRK_ARG(ctx, (uint64_t)first + own <= win->num_batch, "slots [%u, %u) exceed the window's %u", first, first + own, win->num_batch);
    WRK_ARG(ctx, a.num_breakers <= WRK_MAX_DRY_BREAKERS, "%u breakers, at most %u", a.num_breakers, (uint32_t)WRK_MAX_DRY_BREAKERS);
    WRK_ARG(ctx, a.num_breakers == 0 || a.breakers, "num_dry_breakers %u, dry_breakers is NULL", a.num_breakers);
    brk = wrk::DryBreakers{};
    brk.count = a.num_breakers;
    for (uint32_t k = 0; k < a.num_breakers; ++k) {
        WRK_ARG(ctx, a.breakers[k] < V, "breaker %u: id %u >= vocab %u", k, a.breakers[k], V);
        brk.ids[k] = a.breakers[k];
    }
    rows.assign(n, wrk::DryParam{});
    for (uint32_t r = 0; r < n; ++r) {
        const float mult = a.multiplier ? a.multiplier[r] : 0.0f, base = a.base ? a.base[r] : 1.75f;
        const uint32_t allowed = a.allowed_length ? a.allowed_length[r] : 2u, nr = a.no_repeat_ngram ? a.no_repeat_ngram[r] : 0u;
        WRK_ARG(ctx, finite_f32(mult) && mult >= 0.0f, "dry_multiplier[%u] = %g: must be finite and >= 0", r, (double)mult);
        WRK_ARG(ctx, finite_f32(base) && base >= 1.0f, "dry_base[%u] = %g: must be finite and >= 1", r, (double)base);
        WRK_ARG(ctx, allowed >= 1 && allowed <= WRK_DRY_MAX_MATCH, "dry_allowed_length[%u] = %u: must be in [1, %u]", r, allowed,
                (uint32_t)WRK_DRY_MAX_MATCH);
        WRK_ARG(ctx, nr == 0 || (nr >= 2 && nr <= WRK_DRY_MAX_MATCH + 1), "no_repeat_ngram[%u] = %u: 0, or in [2, %u]", r, nr,
                (uint32_t)WRK_DRY_MAX_MATCH + 1);
        wrk::DryParam& p = rows[r];
        const uint32_t slot = first + (r < slots ? r : 0);
        p.ring = win->ring + (size_t)slot * win->capacity;
        p.meta = win->meta + (size_t)slot * 2;
        p.cap = win->capacity;
        p.allowed = allowed; p.no_repeat = nr; p.multiplier = mult;
        dry_penalty_table(mult, base, allowed, p.pen);
    }
    return WRK_OK;
}

// the slot's (length, next write position), read from the device
static int32_t window_meta(wrk_ctx* ctx, const wrk_token_window* win, uint32_t b, uint32_t (&meta)[2]) {
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    WRK_HIP(ctx, hipMemcpyAsync(meta, win->meta + (size_t)b * 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (meta[0] > win->capacity || meta[1] >= win->capacity)
        return wrk_fail(ctx, WRK_E_HIP, "slot %u: inconsistent window (length %u position %u capacity %u)", b, meta[0], meta[1], win->capacity);
    return WRK_OK;
}

static int32_t window_slot_check(wrk_ctx* ctx, const wrk_token_window* win, uint32_t b, const char* who) {
    WRK_ARG(ctx, !ctx->capturing_here(), "%s is blocking: not inside a capture", who);
    WRK_ARG(ctx, win->ctx == ctx, "the token window belongs to another context");
    WRK_ARG(ctx, b < win->num_batch, "slot %u >= %u", b, win->num_batch);
    return WRK_OK;
}

extern "C" {

int32_t wrk_token_window_create(wrk_ctx* ctx, uint32_t B, uint32_t V, uint32_t capacity, wrk_token_window** out) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, B >= 1 && B <= 65535, "num_batch %u: must be in [1, 65535]", B);
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, capacity >= 1 && capacity <= WRK_MAX_TOKEN_WINDOW, "capacity %u: must be in [1, %u]", capacity, (uint32_t)WRK_MAX_TOKEN_WINDOW);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_layout lay;
    const size_t o_r = lay.add((size_t)B * capacity * 4), o_m = lay.add((size_t)B * 8);
    void* mem = nullptr;
    WRK_HIP(ctx, hipMalloc(&mem, lay.total));
    wrk_token_window* win = new wrk_token_window;
    win->ctx = ctx;
    win->num_batch = B; win->num_vocab = V; win->capacity = capacity;
    win->mem = mem;
    win->ring = (uint32_t*)((char*)mem + o_r);
    win->meta = (uint32_t*)((char*)mem + o_m);
    hipError_t e = hipMemsetAsync(mem, 0, lay.total, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        wrk_token_window_destroy(win);
        return wrk_fail(ctx, WRK_E_HIP, "token window: %s", hipGetErrorString(e));
    }
    *out = win;
    return WRK_OK;
}

int32_t wrk_token_window_destroy(wrk_token_window* win) {
    if (!win) return WRK_E_ARG;
    {
        std::lock_guard<std::recursive_mutex> lk(win->ctx->mu);
        hipSetDevice(win->ctx->device);
        hipStreamSynchronize(win->ctx->stream);     // no step in flight still reads the window
        hipFree(win->mem);
    }
    delete win;
    return WRK_OK;
}

int32_t wrk_token_window_add(wrk_ctx* ctx, wrk_token_window* win, uint32_t b, const uint32_t* tokens, uint32_t n) {
    if (!ctx || !win) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = window_slot_check(ctx, win, b, "wrk_token_window_add");
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, n == 0 || tokens, "tokens required");
    for (uint32_t i = 0; i < n; ++i) WRK_ARG(ctx, tokens[i] < win->num_vocab, "token %u: id %u >= vocab %u", i, tokens[i], win->num_vocab);
    if (n == 0) return WRK_OK;
    uint32_t meta[2];
    rc = window_meta(ctx, win, b, meta);
    if (rc != WRK_OK) return rc;
    // only the last `capacity` pushes leave a trace; they land at consecutive ring positions, in at most two pieces
    const uint32_t cap = win->capacity, skip = n > cap ? n - cap : 0, m = n - skip;
    uint32_t pos = (uint32_t)(((uint64_t)meta[1] + skip) % cap);
    uint32_t* ring = win->ring + (size_t)b * cap;
    const uint32_t head = m < cap - pos ? m : cap - pos;
    rc = wrk_buf_write_raw(ctx, ring + pos, tokens + skip, (size_t)head * 4);
    if (rc == WRK_OK && m > head) rc = wrk_buf_write_raw(ctx, ring, tokens + skip + head, (size_t)(m - head) * 4);
    if (rc != WRK_OK) return rc;
    meta[0] = (uint64_t)meta[0] + n < cap ? meta[0] + n : cap;
    meta[1] = (pos + m) % cap;
    rc = wrk_buf_write_raw(ctx, win->meta + (size_t)b * 2, meta, 8);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_token_window_back(wrk_ctx* ctx, const wrk_token_window* win, uint32_t b, uint32_t* tokens_out, uint32_t* len) {
    if (!ctx || !win) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = window_slot_check(ctx, win, b, "wrk_token_window_back");
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, tokens_out && len, "tokens_out and len are required");
    uint32_t meta[2];
    rc = window_meta(ctx, win, b, meta);
    if (rc != WRK_OK) return rc;
    const uint32_t cap = win->capacity, n = meta[0];
    std::vector<uint32_t> ring(cap);
    WRK_HIP(ctx, hipMemcpyAsync(ring.data(), win->ring + (size_t)b * cap, (size_t)cap * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t start = (meta[1] + cap - n) % cap;
    for (uint32_t j = 0; j < n; ++j) tokens_out[j] = ring[(start + j) % cap];
    *len = n;
    return WRK_OK;
}

int32_t wrk_token_window_load(wrk_ctx* ctx, wrk_token_window* win, uint32_t b, const uint32_t* tokens, uint32_t n) {
    if (!ctx || !win) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = window_slot_check(ctx, win, b, "wrk_token_window_load");
    if (rc != WRK_OK) return rc;
    if (!tokens) n = 0;
    WRK_ARG(ctx, n <= win->capacity, "%u tokens, the window holds %u", n, win->capacity);
    for (uint32_t i = 0; i < n; ++i) WRK_ARG(ctx, tokens[i] < win->num_vocab, "token %u: id %u >= vocab %u", i, tokens[i], win->num_vocab);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    if (n) rc = wrk_buf_write_raw(ctx, win->ring + (size_t)b * win->capacity, tokens, (size_t)n * 4);
    const uint32_t meta[2] = {n, n % win->capacity};
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, win->meta + (size_t)b * 2, meta, 8);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_dry_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const wrk_token_window* win, uint32_t first,
                       const float* multiplier, const float* base, const uint32_t* allowed_length, const uint32_t* no_repeat_ngram,
                       const uint32_t* breakers, uint32_t num_breakers) {
    if (!ctx || !logits || !win) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_dry_logits", wrk::SAMPLE_MAX_VOCAB);
    std::vector<wrk::DryParam> rows;
    wrk::DryBreakers brk;
    const wrk_dry_args a{const_cast<wrk_token_window*>(win), multiplier, base, allowed_length, no_repeat_ngram, breakers, num_breakers};
    if (rc == WRK_OK) rc = wrk_dry_pack(ctx, a, first, n, n, V, rows, brk);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add((size_t)n * sizeof(wrk::DryParam)), o_brk = dev.add(sizeof brk), o_scr = dev.add((size_t)n * V * 4);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), rows.data(), (size_t)n * sizeof(wrk::DryParam), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_brk), &brk, sizeof brk, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemsetAsync(dev.at<char>(o_scr), 0, (size_t)n * V * 4, ctx->stream));
    wrk::dry_rows(ctx->stream, (float*)logits->ptr, V, stride, n, dev.at<wrk::DryParam>(o_par), dev.at<wrk::DryBreakers>(o_brk), dev.at<uint32_t>(o_scr));
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

}  // extern "C"
