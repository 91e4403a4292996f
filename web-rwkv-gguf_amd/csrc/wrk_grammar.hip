// Constrained decoding on the device for gfx950: a deterministic automaton over token ids restricts which tokens a row may draw
// (ai00's BNF sampler, vLLM's guided_choice / guided_regex, llama.cpp's grammars, below their compilers).  See DESIGN.md §7k.
//
// A grammar (wrk_grammar) is a DFA with alphabet compression: token_class[V] (u16) maps every token to one of C classes and
// transitions[S][C] (u16) holds the next state, or GRAMMAR_REJECT when the class is not allowed in that state.  A row in state s is
// masked as
//   x'[n] = x[n] (bits unchanged, NaN payloads included) if transitions[s][token_class[n]] != REJECT, else -inf
// and a drawn token y moves it to transitions[s][token_class[y]]; a rejected token leaves it where it was.
//
//   constrain_rows   grid (spans, rows): a workgroup stages its row's transition row (C <= 8192 u16: at most 16 KB) in LDS once and then
//                    masks GRAM_TILES tiles of 1024 tokens, so that the staging is paid once per 4096 tokens and a 65 536-token row still
//                    spreads over 16 workgroups.  VEC: 16-byte logit loads and stores, 8-byte class loads
//   grammar_advance  one row per thread, under the step's RowGate: a row whose draw does not count keeps its state
//
// Everything of the grammar reaches the kernels through a GrammarParam block in device memory, so a captured step program holds no
// table pointer of its own.  Plain vector loads and stores only; no atomics; no kernel waits on another.
#include "wrk_rows_dev.h"
#include "wrk_runner.h" // wrk_buf_write_raw

namespace wrk {

static constexpr uint32_t GRAM_THREADS = 256;
static constexpr uint32_t GRAM_TILE = GRAM_THREADS * 4;        // tokens of one tile: 4 per thread
static constexpr uint32_t GRAM_TILES = 4;                      // tiles per workgroup
static constexpr uint32_t GRAM_SPAN = GRAM_TILE * GRAM_TILES;  // tokens per workgroup
static constexpr uint32_t NEG_INF_BITS = 0xFF800000u;

// VEC: every row of src / dst starts 16-byte aligned and v % 4 == 0 (token_class is 256-byte aligned: its 4 classes at a multiple of 4
// are one 8-byte load), so thread tid owns the 4 tokens at a + 4 * tid of each tile; otherwise it owns a + tid + 256 * j (j < 4), one
// coalesced scalar access each.  Logits move as u32: no float operation touches them.  src and dst may be the same rows (in place): a
// thread reads exactly the elements it writes.
template <bool VEC>
__global__ void __launch_bounds__(GRAM_THREADS) constrain_rows_kernel(const uint32_t* src, uint32_t v, uint32_t src_stride,
                                                                      const GrammarParam* __restrict__ par, uint32_t* dst, uint32_t dst_stride) {
    __shared__ uint16_t next[WRK_MAX_TOKEN_CLASSES];
    const uint32_t r = blockIdx.y, tid = threadIdx.x;
    const GrammarParam p = *par;
    const uint32_t nc = p.num_classes < WRK_MAX_TOKEN_CLASSES ? p.num_classes : WRK_MAX_TOKEN_CLASSES;
    const uint16_t* trow = p.transitions + (size_t)p.states[r] * p.num_classes;
    for (uint32_t c = tid; c < nc; c += GRAM_THREADS) next[c] = trow[c];
    __syncthreads();
    const uint32_t* x = src + (size_t)r * src_stride;
    uint32_t* y = dst + (size_t)r * dst_stride;
    const uint32_t a0 = blockIdx.x * GRAM_SPAN;
    if (VEC) {
        u32x4 xv[GRAM_TILES];
        u32x2 cv[GRAM_TILES];
#pragma unroll
        for (uint32_t k = 0; k < GRAM_TILES; ++k) {
            const uint32_t i = a0 + k * GRAM_TILE + tid * 4;
            if (i < v) {
                xv[k] = *(const u32x4*)(x + i);
                cv[k] = *(const u32x2*)(p.token_class + i);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < GRAM_TILES; ++k) {
            const uint32_t i = a0 + k * GRAM_TILE + tid * 4;
            if (i >= v) continue;
            u32x4 o;
            o.x = next[cv[k].x & 0xffffu] != WRK_GRAMMAR_REJECT ? xv[k].x : NEG_INF_BITS;
            o.y = next[cv[k].x >> 16] != WRK_GRAMMAR_REJECT ? xv[k].y : NEG_INF_BITS;
            o.z = next[cv[k].y & 0xffffu] != WRK_GRAMMAR_REJECT ? xv[k].z : NEG_INF_BITS;
            o.w = next[cv[k].y >> 16] != WRK_GRAMMAR_REJECT ? xv[k].w : NEG_INF_BITS;
            *(u32x4*)(y + i) = o;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < GRAM_TILES; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = a0 + k * GRAM_TILE + j * GRAM_THREADS + tid;
                if (i < v) y[i] = next[p.token_class[i]] != WRK_GRAMMAR_REJECT ? x[i] : NEG_INF_BITS;
            }
    }
}

// a row whose draw does not count returns before it reads anything else of its row; a token outside the vocabulary (none reaches here:
// the picks return ids < v) is treated as rejected
__global__ void __launch_bounds__(GRAM_THREADS) grammar_advance_kernel(uint32_t v, uint32_t n, const GrammarParam* __restrict__ par,
                                                                       const uint32_t* __restrict__ tokens, const RowGate gate) {
    const uint32_t r = blockIdx.x * GRAM_THREADS + threadIdx.x;
    if (r >= n || !row_counts(gate, r)) return;
    const GrammarParam p = *par;
    const uint32_t t = tokens[r];
    if (t >= v) return;
    const uint32_t s = p.states[r];
    const uint16_t nx = p.transitions[(size_t)s * p.num_classes + p.token_class[t]];
    if (nx != WRK_GRAMMAR_REJECT) p.states[r] = nx;
}

void constrain_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, const GrammarParam* par, float* dst,
                    uint32_t dst_stride) {
    if (n == 0 || v == 0) return;
    const dim3 grid((v + GRAM_SPAN - 1) / GRAM_SPAN, n);
    if (v % 4 == 0 && src_stride % 4 == 0 && dst_stride % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0)
        constrain_rows_kernel<true><<<grid, GRAM_THREADS, 0, s>>>((const uint32_t*)src, v, src_stride, par, (uint32_t*)dst, dst_stride);
    else constrain_rows_kernel<false><<<grid, GRAM_THREADS, 0, s>>>((const uint32_t*)src, v, src_stride, par, (uint32_t*)dst, dst_stride);
}

void grammar_advance(hipStream_t s, uint32_t v, uint32_t n, const GrammarParam* par, const uint32_t* tokens, const RowGate& gate) {
    if (n == 0 || v == 0) return;
    grammar_advance_kernel<<<(n + GRAM_THREADS - 1) / GRAM_THREADS, GRAM_THREADS, 0, s>>>(v, n, par, tokens, gate);
}

}  // namespace wrk

wrk::GrammarParam wrk_grammar::param(uint32_t* states) const { return wrk::GrammarParam{token_class, transitions, num_classes, 0u, states}; }

int32_t wrk_grammar_pack(wrk_ctx* ctx, const wrk_grammar* g, const uint32_t* state, uint32_t n, uint32_t V, std::vector<uint32_t>& out) {
    WRK_ARG(ctx, g, "grammar required");
    WRK_ARG(ctx, g->ctx == ctx, "the grammar belongs to another context");
    WRK_ARG(ctx, g->num_vocab == V, "grammar of %u tokens, logits of %u", g->num_vocab, V);
    out.assign(n, 0u);
    for (uint32_t r = 0; r < n && state; ++r) {
        WRK_ARG(ctx, state[r] < g->num_states, "grammar_state[%u] = %u: the grammar has %u states", r, state[r], g->num_states);
        out[r] = state[r];
    }
    return WRK_OK;
}

extern "C" {

int32_t wrk_grammar_create(wrk_ctx* ctx, uint32_t V, uint32_t S, uint32_t NC, const uint16_t* token_class, const uint16_t* transitions,
                           wrk_grammar** out) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, S >= 1 && S <= 65535, "num_states %u: must be in [1, 65535]", S);
    WRK_ARG(ctx, NC >= 1 && NC <= WRK_MAX_TOKEN_CLASSES, "num_classes %u: must be in [1, %u]", NC, (uint32_t)WRK_MAX_TOKEN_CLASSES);
    WRK_ARG(ctx, token_class && transitions, "token_class and transitions are required");
    std::vector<uint8_t> used(NC, 0);       // classes that at least one token maps to
    for (uint32_t t = 0; t < V; ++t) {
        WRK_ARG(ctx, token_class[t] < NC, "token_class[%u] = %u >= %u classes", t, token_class[t], NC);
        used[token_class[t]] = 1;
    }
    for (uint32_t s = 0; s < S; ++s) {
        bool any = false;
        for (uint32_t c = 0; c < NC; ++c) {
            const uint16_t nx = transitions[(size_t)s * NC + c];
            WRK_ARG(ctx, nx < S || nx == WRK_GRAMMAR_REJECT, "transitions[%u][%u] = %u: neither a state (< %u) nor WRK_GRAMMAR_REJECT", s, c, nx, S);
            any |= nx != WRK_GRAMMAR_REJECT && used[c];
        }
        WRK_ARG(ctx, any, "state %u allows no token", s);
    }
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_layout lay;
    const size_t o_c = lay.add((size_t)V * 2), o_t = lay.add((size_t)S * NC * 2);
    void* mem = nullptr;
    WRK_HIP(ctx, hipMalloc(&mem, lay.total));
    wrk_grammar* g = new wrk_grammar;
    g->ctx = ctx;
    g->num_vocab = V; g->num_states = S; g->num_classes = NC;
    g->mem = mem;
    g->token_class = (uint16_t*)((char*)mem + o_c);
    g->transitions = (uint16_t*)((char*)mem + o_t);
    int32_t rc = wrk_buf_write_raw(ctx, g->token_class, token_class, (size_t)V * 2);
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, g->transitions, transitions, (size_t)S * NC * 2);
    if (rc == WRK_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = wrk_fail(ctx, WRK_E_HIP, "grammar upload failed");
    if (rc != WRK_OK) { wrk_grammar_destroy(g); return rc; }
    *out = g;
    return WRK_OK;
}

int32_t wrk_grammar_destroy(wrk_grammar* g) {
    if (!g) return WRK_E_ARG;
    {
        std::lock_guard<std::recursive_mutex> lk(g->ctx->mu);
        hipSetDevice(g->ctx->device);
        hipStreamSynchronize(g->ctx->stream);       // no step in flight still reads the tables
        hipFree(g->mem);
    }
    delete g;
    return WRK_OK;
}

int32_t wrk_constrain_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const wrk_grammar* g, const uint32_t* states) {
    if (!ctx || !logits || !g) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, n, "wrk_constrain_logits", wrk::SAMPLE_MAX_VOCAB);
    std::vector<uint32_t> st;
    if (rc == WRK_OK) WRK_ARG(ctx, n == 0 || states, "states required");
    if (rc == WRK_OK) rc = wrk_grammar_pack(ctx, g, states, n, V, st);
    if (rc != WRK_OK || n == 0) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::GrammarParam)), o_st = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    const wrk::GrammarParam par = g->param(dev.at<uint32_t>(o_st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_st), st.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::constrain_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, dev.at<wrk::GrammarParam>(o_par), (float*)logits->ptr, stride);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_grammar_advance(wrk_ctx* ctx, const wrk_grammar* g, uint32_t* states, const uint32_t* tokens, uint32_t n) {
    if (!ctx || !g) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_grammar_advance is blocking: not inside a capture");
    WRK_ARG(ctx, n == 0 || (states && tokens), "states and tokens are required");
    std::vector<uint32_t> st;
    const int32_t rc = wrk_grammar_pack(ctx, g, states, n, g->num_vocab, st);
    if (rc != WRK_OK || n == 0) return rc;
    for (uint32_t r = 0; r < n; ++r) WRK_ARG(ctx, tokens[r] < g->num_vocab, "token %u: id %u >= vocab %u", r, tokens[r], g->num_vocab);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::GrammarParam)), o_st = dev.add((size_t)n * 4), o_tok = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    const wrk::GrammarParam par = g->param(dev.at<uint32_t>(o_st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_st), st.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tok), tokens, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::grammar_advance(ctx->stream, g->num_vocab, n, dev.at<wrk::GrammarParam>(o_par), dev.at<uint32_t>(o_tok), wrk::RowGate{nullptr, 0u, 0u});
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(states, dev.at<char>(o_st), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

}  // extern "C"
