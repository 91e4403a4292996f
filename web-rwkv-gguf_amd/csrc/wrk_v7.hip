// RWKV-7 model runner behind wrk_v7_* (include/wrk_hip.h).
//
// mode 0 ("op-by-op") enqueues exactly the TensorOp list that v7::Bundle::dispatch builds
// (src/runtime/v7.rs:598-713, dispatch_layer :716-1007, dispatch_header :1009-1036), one kernel per
// reference op, on scratch buffers laid out like `Runtime<f16>` (v7.rs:281-364).
// mode 1 ("fused") runs the decode fast path of wrk_v7_fused.hip when every sequence of the chunk
// contributes exactly one token, and falls back to mode 0 otherwise (prefill chunks).
#include "wrk_internal.h"
#include "wrk_v7.h"
#include "wrk_v7_engine.h"

#define LOCK(ctx) std::lock_guard<std::recursive_mutex> _lk((ctx)->mu)

static constexpr float LN_EPS = 1.0e-5f;    // v7.rs:47
static constexpr float GN_EPS = 64.0e-5f;   // v7.rs:48
static constexpr float L2_EPS = 1.0e-12f;   // v7.rs:46

using wrk::mat_job;

// ------------------------------------------------------------------ scratch ("Runtime<f16>" + "Header<f16>")
int32_t wrk_v7_model::ensure_scratch(uint32_t T, uint32_t NH) {
    if (T <= scratch_tokens && NH <= scratch_headers && scratch) return WRK_OK;
    if (ctx->capturing_here()) return wrk_fail(ctx, WRK_E_ARG, "scratch must be sized before capture");
    const uint32_t nt = T > scratch_tokens ? T : scratch_tokens;
    const uint32_t nh = NH > scratch_headers ? NH : scratch_headers;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    drop_graphs();                                   // captured graphs hold the old pointers
    if (scratch) hipFree(scratch);
    scratch = nullptr;
    const size_t D = d.num_emb, F = d.num_hidden, V = d.num_vocab;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += wrk_up256(bytes); return o; };
    const size_t esz = act_dtype == WRK_F32 ? 4 : 2;        // Runtime<F>: every buffer but `input` holds F
    const size_t vecT = D * nt * esz;
    size_t o_named[32];
    int ni = 0;
    for (int i = 0; i < 23; ++i) o_named[ni++] = take(vecT);          // input, x, att_x, att_v0, 6 shifted, r w k v a g o, kk, vv, ffn_x, ffn_kx, ffn_v, spare
    const size_t o_n = take(vecT * 4);
    const size_t o_auxw = take((size_t)d.lora_w * nt * esz), o_auxa = take((size_t)d.lora_a * nt * esz);
    const size_t o_auxg = take((size_t)d.lora_g * nt * esz), o_auxv = take((size_t)d.lora_v * nt * esz);
    const size_t o_ffnk = take(F * nt * esz);
    const size_t o_headx = take(D * nh * esz), o_heado = take(V * nh * 4);
    const size_t o_cur = take((size_t)nt * 4), o_tok = take((size_t)nt * 4), o_hdr = take((size_t)nh * 4), o_arg = take((size_t)nh * 4);
    const size_t o_cnt = take(256);
    // K-sliced GEMM (decode batches of 2 .. 64 tokens): f32 partial tiles [row group][K slice][token][64 rows] of the largest launch of a
    // layer (at most one slice per 256-block) and one arrival counter per row group
    size_t ks_floats = 0, ks_groups = 0, o_ksp = 0, o_ksc = 0;
    if (nt >= 2 && act_dtype == WRK_F16) {       // (a frame sized for longer chunks still serves decode batches of up to 64)
        const size_t ntp = nt <= 16 ? 16 : (nt <= 32 ? 32 : 64);
        auto tiles = [](size_t m, size_t k) { return ((m + 63) / 64) * (k / 256 ? k / 256 : 1); };
        auto groups = [](size_t m) { return (m + 63) / 64; };
        const size_t lora = tiles(d.lora_w, D) + tiles(d.lora_a, D) + tiles(d.lora_g, D) + tiles(d.lora_v, D);
        const size_t k1 = 3 * tiles(D, D) + lora, k5 = tiles(F, D), k6 = tiles(D, F);
        const size_t most = k1 > k5 ? (k1 > k6 ? k1 : k6) : (k5 > k6 ? k5 : k6);
        ks_floats = most * 64 * ntp;
        ks_groups = 3 * groups(D) + groups(d.lora_w) + groups(d.lora_a) + groups(d.lora_g) + groups(d.lora_v) + groups(F) + 8;
        o_ksp = take(ks_floats * 4);
        o_ksc = take(ks_groups * 4);
    }
    WRK_HIP(ctx, hipMalloc(&scratch, off));
    WRK_HIP(ctx, hipMemsetAsync(scratch, 0, off, ctx->stream));
    if (nt >= 128 && act_dtype == WRK_F16) {
        // prefill GEMM (wrk_gemm3.hip): sub-block input sums of the stacked tokens, hi + lo f16 per 32 inputs, for the up to three distinct
        // inputs of a launch (r, k, v) or the F-wide ffn vector; + the f32 partial tiles of K-split launches (chunks of up to 256 tokens:
        // the widest launch, r / k / v or the ffn key, in two to four slices)
        const size_t widest = std::max<size_t>(3 * D, F);
        const size_t part = (size_t)256 * widest * 4 * 4;
        const int32_t rs = wrk_ctx_reserve_gemm_scratch(ctx, (size_t)nt * (widest / 32) * 4 + 3 * ((size_t)nt * 4 + 256) /* per-token factors of the sums */ + 8 * 1024 + part);
        if (rs != WRK_OK) return rs;
    }
    char* b = (char*)scratch;
    ni = 0;
    s.input = b + o_named[ni++]; s.x = b + o_named[ni++]; s.att_x = b + o_named[ni++]; s.att_v0 = b + o_named[ni++];
    s.rx = b + o_named[ni++]; s.wx = b + o_named[ni++]; s.kx = b + o_named[ni++]; s.vx = b + o_named[ni++];
    s.ax = b + o_named[ni++]; s.gx = b + o_named[ni++];
    s.r = b + o_named[ni++]; s.w = b + o_named[ni++]; s.k = b + o_named[ni++]; s.v = b + o_named[ni++];
    s.a = b + o_named[ni++]; s.g = b + o_named[ni++]; s.o = b + o_named[ni++];
    s.kk = b + o_named[ni++]; s.vv = b + o_named[ni++];
    s.ffn_x = b + o_named[ni++]; s.ffn_kx = b + o_named[ni++]; s.ffn_v = b + o_named[ni++]; s.ln_tmp = b + o_named[ni++];
    s.n = b + o_n;
    s.aux_w = b + o_auxw; s.aux_a = b + o_auxa; s.aux_g = b + o_auxg; s.aux_v = b + o_auxv;
    s.ffn_k = b + o_ffnk;
    s.head_x = b + o_headx; s.head_o = (float*)(b + o_heado);
    s.cursors = (uint32_t*)(b + o_cur); s.tokens = (uint32_t*)(b + o_tok); s.headers = (uint32_t*)(b + o_hdr); s.argmax = (uint32_t*)(b + o_arg);
    s.counter = (uint32_t*)(b + o_cnt);
    s.ks_part = ks_floats ? (float*)(b + o_ksp) : nullptr; s.ks_cnt = ks_floats ? (uint32_t*)(b + o_ksc) : nullptr;
    s.ks_part_cap = ks_floats; s.ks_cnt_cap = (uint32_t)ks_groups;
    scratch_tokens = nt;
    scratch_headers = nh;
    // arg-max partials of the head matvec: one (value, index) per workgroup and header row
    {
        wrk::MatJob hj = mat_job(head, make_dense(s.head_x, WRK_F16, d.num_emb, nh), make_dense(s.head_o, WRK_F32, d.num_vocab, nh), 0);
        const size_t need = (size_t)wrk::matvec_num_wg(&hj, 1, ctx->num_cu, nullptr) * nh;
        if (need > amax_cap) {
            free_fused();
            WRK_HIP(ctx, hipMalloc((void**)&amax_val, need * 4));
            WRK_HIP(ctx, hipMalloc((void**)&amax_idx, need * 4));
            amax_cap = need;
        }
    }
    return WRK_OK;
}

#define MM(...)                                   \
    do {                                          \
        int32_t _r = wrk_mm(ctx, __VA_ARGS__);    \
        if (_r != WRK_OK) return _r;              \
    } while (0)

// ------------------------------------------------------------------ mode 0: the reference op list
int32_t wrk_v7_model::enqueue_ops(wrk_v7_state* st, uint32_t T, uint32_t NH, bool identity_headers, bool merged) {
    hipStream_t q = ctx->op_stream();
    const uint32_t D = d.num_emb, F = d.num_hidden, H = d.num_head, S = D / H, V = d.num_vocab;
    const uint32_t AT = act_dtype;      // F of Runtime<F>
    if (AT != WRK_F16) merged = false;  // the merged launches are written for dense f16 rows
    auto vec = [&](void* p, uint32_t c = 0) { return make_dense(p, AT, c ? c : D, T); };
    auto heads = [&](void* p) { return make_dense(p, AT, S, H, T); };
    DTensor x = vec(s.x), att_x = vec(s.att_x), v0 = vec(s.att_v0);
    DTensor rx = vec(s.rx), wx = vec(s.wx), kx = vec(s.kx), vx = vec(s.vx), ax = vec(s.ax), gx = vec(s.gx);
    DTensor r = vec(s.r), w = vec(s.w), k = vec(s.k), v = vec(s.v), a = vec(s.a), g = vec(s.g), o = vec(s.o);
    DTensor kk = vec(s.kk), vv = vec(s.vv);
    DTensor ffn_x = vec(s.ffn_x), ffn_kx = vec(s.ffn_kx), ffn_v = vec(s.ffn_v), ffn_k = vec(s.ffn_k, F);
    DTensor aux_w = vec(s.aux_w, d.lora_w), aux_a = vec(s.aux_a, d.lora_a), aux_g = vec(s.aux_g, d.lora_g), aux_v = vec(s.aux_v, d.lora_v);
    DTensor n4 = make_dense(s.n, AT, S, H, T, 4);
    auto nslice = [&](uint32_t i) { DTensor t = make_dense(s.n, AT, D, T, 4); t.shape[2] = 1; t.offset[2] = i; return t; };
    auto bvec = [&](const wrk_buf* b) { return make_dense(b->ptr, WRK_F16, D, 1, 1); };
    // WRK_MERGE_MASK (debug): 1 shifts in one pass, 2 grouped projections, 4 pre-WKV stage, 8 post-WKV stage, 16 W_o add in the epilogue,
    // 32 blit + layer_norm in one pass, 64 ffn.value's add in the epilogue
    const char* mm_env = getenv("WRK_MERGE_MASK");
    const unsigned mask = mm_env ? (unsigned)atoi(mm_env) : 127u;
    const bool wide = merged && S == 64 && T > 0;     // merged element-wise stages (one wave per head and token)
    const bool m_shift = merged && (mask & 1u), m_group = merged && (mask & 2u), m_pre = wide && (mask & 4u), m_post = wide && (mask & 8u),
               m_res = merged && (mask & 16u), m_ln = merged && (mask & 32u), m_tail = merged && (mask & 64u);

    // embed: LN(ln0) in place on the gathered rows, blit to x (v7.rs:649-659)
    if (!skip_embed) {
        DTensor input = make_dense(s.input, WRK_F16, D, T);     // Runtime::input is f16 whatever F is (v7.rs:283)
        wrk::layer_norm(q, ln0_w->ptr, ln0_b->ptr, input, LN_EPS);
        wrk::blit(q, input, x);
    }

    for (uint32_t li = layer_begin; li < d.num_layer && li < layer_end; ++li) {
        const wrk_v7_layer_desc& L = layers[li];
        // state views (v7.rs:198-208): att = rows 0..S, ffn = row S+1 of [D, S+2, B]
        DTensor st_att = make_dense(st->layer_ptr(li), WRK_F32, D, S + 2, st->num_batch);
        st_att.shape[1] = S + 1;
        DTensor st_row0 = st_att; st_row0.shape[1] = 1;
        DTensor st_ffn = make_dense(st->layer_ptr(li), WRK_F32, D, S + 2, st->num_batch);
        st_ffn.shape[1] = 1; st_ffn.offset[1] = S + 1;

        if (m_ln) wrk::layer_norm_from(q, L.ln1_w->ptr, L.ln1_b->ptr, x, att_x, LN_EPS);     // 1-2 in one pass
        else {
            wrk::blit(q, x, att_x);                                                      // 1
            wrk::layer_norm(q, L.ln1_w->ptr, L.ln1_b->ptr, att_x, LN_EPS);               // 2
        }
        // Mode 1 (merged): same arithmetic, fewer launches for multi-token chunks -- the six shifts read LN(x) once, the projections
        // that are ready together share a launch (r, k, v, LoRA downs | LoRA ups), the element-wise chains run as one kernel.
        if (m_shift) {
            const DTensor mixes[6] = {bvec(L.x_r), bvec(L.x_w), bvec(L.x_k), bvec(L.x_v), bvec(L.x_a), bvec(L.x_g)};
            const DTensor outs[6] = {rx, wx, kx, vx, ax, gx};
            wrk::token_shift_multi(q, s.cursors, mixes, outs, 6, st_row0, att_x, 1);
        } else {
            wrk::token_shift(q, s.cursors, bvec(L.x_r), st_row0, att_x, rx, 1);               // 3
            wrk::token_shift(q, s.cursors, bvec(L.x_w), st_row0, att_x, wx, 1);
            wrk::token_shift(q, s.cursors, bvec(L.x_k), st_row0, att_x, kx, 1);
            wrk::token_shift(q, s.cursors, bvec(L.x_v), st_row0, att_x, vx, 1);
            wrk::token_shift(q, s.cursors, bvec(L.x_a), st_row0, att_x, ax, 1);
            wrk::token_shift(q, s.cursors, bvec(L.x_g), st_row0, att_x, gx, 1);
        }
        if (m_group) {
            wrk::MatJob ja[7] = {mat_job(L.w_r, rx, r, WRK_ACT_NONE), mat_job(L.w_k, kx, k, WRK_ACT_NONE), mat_job(L.w_v, vx, v, WRK_ACT_NONE),
                                 mat_job(L.w1, wx, aux_w, WRK_ACT_TANH), mat_job(L.a1, ax, aux_a, WRK_ACT_NONE), mat_job(L.g1, gx, aux_g, WRK_ACT_SIGMOID),
                                 mat_job(li ? L.v1 : L.a1, li ? vx : ax, li ? aux_v : aux_a, WRK_ACT_NONE)};
            int32_t rg = wrk_mm_group(ctx, ja, li ? 7 : 6);
            if (rg != WRK_OK) return rg;
            wrk::MatJob jb[4] = {mat_job(L.w2, aux_w, w, WRK_ACT_NONE), mat_job(L.a2, aux_a, a, WRK_ACT_NONE), mat_job(L.g2, aux_g, g, WRK_ACT_NONE),
                                 mat_job(li ? L.v2 : L.a2, li ? aux_v : aux_a, li ? vv : a, WRK_ACT_NONE)};
            rg = wrk_mm_group(ctx, jb, li ? 4 : 3);
            if (rg != WRK_OK) return rg;
        } else {
            MM(L.w_r, rx, r, WRK_ACT_NONE);                                                  // 4
            MM(L.w_k, kx, k, WRK_ACT_NONE);
            MM(L.w_v, vx, v, WRK_ACT_NONE);
            MM(L.w1, wx, aux_w, WRK_ACT_TANH);                                               // 5
            MM(L.w2, aux_w, w, WRK_ACT_NONE);
            MM(L.a1, ax, aux_a, WRK_ACT_NONE);                                               // 6
            MM(L.a2, aux_a, a, WRK_ACT_NONE);
            MM(L.g1, gx, aux_g, WRK_ACT_SIGMOID);                                            // 7
            MM(L.g2, aux_g, g, WRK_ACT_NONE);
            if (li) {                                                                        // 10 (projections)
                MM(L.v1, vx, aux_v, WRK_ACT_NONE);
                MM(L.v2, aux_v, vv, WRK_ACT_NONE);
            }
        }
        // (not with many sequences: the one-wave-per-head kernel prepares its decays itself, and 4 D bytes per token would be written for nothing)
        float* wdec = ((size_t)F * (act_dtype == WRK_F32 ? 4 : 2) >= (size_t)4 * D && (size_t)wkv_nseq * H < 768) ? (float*)s.ffn_k : nullptr;
        if (m_pre) {     // steps 5-11's element-wise ops in one launch, bit-identical (wrk_ops.hip: pre_wkv_v7)
            // (the decays of the chunk kernel ride along, f32 [D, T], in the ffn key buffer: 4 D values per token, free until the ffn key GEMM)
            wrk::pre_wkv_v7(q, s.w, s.a, s.k, s.v, s.vv, s.att_v0, s.n, L.w0->ptr, L.a0->ptr, L.k_k->ptr, L.k_a->ptr, li ? L.v0->ptr : L.a0->ptr,
                            D, T, li == 0, L2_EPS, wdec);
        } else {
            wrk::binary(q, 0, bvec(L.w0), w, 0, 0, 0);                                       // 5
            wrk::binary(q, 0, bvec(L.a0), a, 0, 0, WRK_ACT_SIGMOID);                         // 6
            wrk::blit(q, k, kk);                                                             // 8
            wrk::binary(q, 1, bvec(L.k_k), kk, 0, 0, 0);
            wrk::l2_norm(q, heads(s.kk), L2_EPS);
            wrk::control_k_v7(q, L.k_a->ptr, a, k);                                          // 9
            if (li == 0) {                                                                   // 10
                wrk::blit(q, v, v0);
            } else {
                wrk::binary(q, 0, bvec(L.v0), vv, 0, 0, WRK_ACT_SIGMOID);
                wrk::lerp(q, v0, v, vv, 1);
            }
            wrk::blit(q, k, nslice(0));                                                      // 11
            wrk::blit(q, v, nslice(1));
            wrk::blit(q, a, nslice(2));
            wrk::blit(q, kk, nslice(3));
        }
        wrk::time_mix_v7(q, s.cursors, st_att, heads(s.r), heads(s.w), n4, heads(s.att_x), wkv_nseq, m_pre ? wdec : nullptr);   // 12
        if (m_post) wrk::post_wkv_v7(q, s.att_x, s.r, s.g, s.n, L.gn_w->ptr, L.gn_b->ptr, L.r_k->ptr, D, T, GN_EPS);    // 13-15 in one launch
        else {
            wrk::group_norm(q, L.gn_w->ptr, L.gn_b->ptr, heads(s.att_x), GN_EPS);        // 13
            wrk::time_first_v7(q, L.r_k->ptr, heads(s.r), n4, heads(s.att_x));           // 14
            wrk::binary(q, 1, g, att_x, 0, 0, 0);                                        // 15
        }
        if (m_res) {        // the add rides the projection's epilogue: x = round(W_o att_x) + x
            wrk::MatJob jo = mat_job(L.w_o, att_x, x, WRK_ACT_NONE);
            jo.has_res = 1;
            jo.res = x;
            const int32_t rg = wrk_mm_group(ctx, &jo, 1);
            if (rg != WRK_OK) return rg;
        } else {
            MM(L.w_o, att_x, o, WRK_ACT_NONE);                                           // 16
            wrk::binary(q, 0, o, x, 0, 0, 0);
        }
        if (m_ln) wrk::layer_norm_from(q, L.ln2_w->ptr, L.ln2_b->ptr, x, ffn_x, LN_EPS);
        else {
            wrk::blit(q, x, ffn_x);                                                      // 17
            wrk::layer_norm(q, L.ln2_w->ptr, L.ln2_b->ptr, ffn_x, LN_EPS);
        }
        wrk::token_shift(q, s.cursors, bvec(L.ffn_x_k), st_ffn, ffn_x, ffn_kx, 1);        // 18
        MM(L.ffn_w_k, ffn_kx, ffn_k, WRK_ACT_SQUARED_RELU);                              // 19
        if (m_tail) {       // x = round(W_v k) + x in the epilogue; channel_mix still saves the ffn shift state (its copy is dead)
            wrk::MatJob jv = mat_job(L.ffn_w_v, ffn_k, x, WRK_ACT_NONE);
            jv.has_res = 1;
            jv.res = x;
            const int32_t rg = wrk_mm_group(ctx, &jv, 1);
            if (rg != WRK_OK) return rg;
            wrk::channel_mix_v7(q, s.cursors, st_ffn, ffn_v, ffn_x);
        } else {
            MM(L.ffn_w_v, ffn_k, ffn_v, WRK_ACT_NONE);                                   // 20
            wrk::channel_mix_v7(q, s.cursors, st_ffn, ffn_v, ffn_x);                     // 21
            wrk::binary(q, 0, ffn_x, x, 0, 0, 0);                                        // 22
        }
        if ((li + 1) % d.rescale == 0) wrk::affine(q, x, 0.5f, 0.0f);                    // 23
    }
    // header (v7.rs:1009-1036): gather header rows, LN(ln_out), head matmul into f32 logits
    if (NH > 0) {
        DTensor head_x = make_dense(s.head_x, AT, D, NH);
        if (identity_headers) wrk::blit(q, make_dense(s.x, AT, D, NH), head_x);
        else wrk::gather_rows_any(q, x, s.headers, head_x, NH);
        wrk::layer_norm(q, ln_out_w->ptr, ln_out_b->ptr, head_x, LN_EPS);
        MM(head, head_x, make_dense(s.head_o, WRK_F32, V, NH), WRK_ACT_NONE);
    }
    WRK_LAUNCH_CHECK(ctx);
    return WRK_OK;
}

// ------------------------------------------------------------------ C ABI
bool split_head_env_on() { const char* e = getenv("WRK_SPLIT_HEAD"); return !(e && e[0] == '0'); }

extern "C" {

int32_t wrk_v7_model_create(wrk_ctx* ctx, const wrk_v7_model_desc* desc, wrk_v7_model** out) {
    if (!ctx || !desc || !out) return WRK_E_ARG;
    LOCK(ctx);
    *out = nullptr;
    WRK_ARG(ctx, desc->num_layer >= 1 && desc->num_head >= 1 && desc->num_emb % desc->num_head == 0, "bad model dims");
    WRK_ARG(ctx, desc->num_emb / desc->num_head == 64, "head size must be 64");
    WRK_ARG(ctx, desc->layers && desc->head && desc->ln0_w && desc->ln0_b && desc->ln_out_w && desc->ln_out_b, "missing tensors");
    WRK_ARG(ctx, desc->head->k == desc->num_emb && desc->head->m >= desc->num_vocab, "head matrix shape mismatch");
    const uint32_t D = desc->num_emb, F = desc->num_hidden;
    for (uint32_t l = 0; l < desc->num_layer; ++l) {
        const wrk_v7_layer_desc& L = desc->layers[l];
        const wrk_buf* vecs[] = {L.ln1_w, L.ln1_b, L.ln2_w, L.ln2_b, L.x_r, L.x_w, L.x_k, L.x_v, L.x_a, L.x_g, L.w0, L.a0,
                                 L.r_k, L.k_k, L.k_a, L.gn_w, L.gn_b, L.ffn_x_k};
        for (const wrk_buf* b : vecs) WRK_ARG(ctx, b && b->bytes >= (size_t)D * 2, "layer %u: vector missing or shorter than D f16", l);
        struct { const wrk_matrix* m; uint32_t k, mm; } mats[] = {
            {L.w1, D, desc->lora_w}, {L.w2, desc->lora_w, D}, {L.a1, D, desc->lora_a}, {L.a2, desc->lora_a, D},
            {L.g1, D, desc->lora_g}, {L.g2, desc->lora_g, D}, {L.w_k, D, D}, {L.w_v, D, D}, {L.w_r, D, D}, {L.w_o, D, D},
            {L.ffn_w_k, D, F}, {L.ffn_w_v, F, D}};
        for (auto& e : mats) WRK_ARG(ctx, e.m && e.m->k == e.k && e.m->m == e.mm, "layer %u: matrix missing or wrong shape (want K=%u M=%u)", l, e.k, e.mm);
        if (l > 0) {
            WRK_ARG(ctx, L.v0 && L.v0->bytes >= (size_t)D * 2, "layer %u: v0 missing", l);
            WRK_ARG(ctx, L.v1 && L.v1->k == D && L.v1->m == desc->lora_v && L.v2 && L.v2->k == desc->lora_v && L.v2->m == D, "layer %u: v1/v2 wrong shape", l);
        }
    }
    wrk_v7_model* m = new wrk_v7_model();
    m->ctx = ctx;
    m->d = *desc;
    m->d.rescale = desc->rescale ? desc->rescale : 1024;
    m->layers.assign(desc->layers, desc->layers + desc->num_layer);
    m->d.layers = m->layers.data();
    m->ln0_w = desc->ln0_w; m->ln0_b = desc->ln0_b; m->ln_out_w = desc->ln_out_w; m->ln_out_b = desc->ln_out_b;
    m->emb = desc->emb_f16; m->head = desc->head;
    // retain every handle (the Rust side keeps Arc clones inside v7::Model)
    auto rb = [](const wrk_buf* b) { if (b) const_cast<wrk_buf*>(b)->refs.fetch_add(1); };
    auto rm = [](const wrk_matrix* x) { if (x) const_cast<wrk_matrix*>(x)->refs.fetch_add(1); };
    rb(m->ln0_w); rb(m->ln0_b); rb(m->ln_out_w); rb(m->ln_out_b); rb(m->emb); rm(m->head);
    for (auto& L : m->layers) {
        const wrk_buf* vecs[] = {L.ln1_w, L.ln1_b, L.ln2_w, L.ln2_b, L.x_r, L.x_w, L.x_k, L.x_v, L.x_a, L.x_g, L.w0, L.a0, L.v0,
                                 L.r_k, L.k_k, L.k_a, L.gn_w, L.gn_b, L.ffn_x_k};
        for (const wrk_buf* b : vecs) rb(b);
        const wrk_matrix* mats[] = {L.w1, L.w2, L.a1, L.a2, L.g1, L.g2, L.v1, L.v2, L.w_k, L.w_v, L.w_r, L.w_o, L.ffn_w_k, L.ffn_w_v};
        for (const wrk_matrix* x : mats) rm(x);
    }
    *out = m;
    return WRK_OK;
}

int32_t wrk_v7_model_destroy(wrk_v7_model* m) {
    if (!m) return WRK_E_ARG;
    wrk_ctx* ctx = m->ctx;
    {
        LOCK(ctx);
        hipSetDevice(ctx->device);
        hipStreamSynchronize(ctx->stream);
        for (hipStream_t s : m->lane_streams) { hipStreamSynchronize(s); hipStreamDestroy(s); }
        m->release_common();
        m->free_fused();
        wrk_v7_engine_destroy(m->engine);
        m->engine = nullptr;
        for (hipEvent_t e : m->lane_events) hipEventDestroy(e);
        m->lane_streams.clear(); m->lane_events.clear();
    }
    for (wrk_v7_model* lane : m->lanes) wrk_v7_model_destroy(lane);
    m->lanes.clear();
    auto fb = [](const wrk_buf* b) { if (b) wrk_buf_release(const_cast<wrk_buf*>(b)); };
    auto fm = [](const wrk_matrix* x) { if (x) wrk_matrix_release(const_cast<wrk_matrix*>(x)); };
    fb(m->ln0_w); fb(m->ln0_b); fb(m->ln_out_w); fb(m->ln_out_b); fb(m->emb); fm(m->head);
    for (auto& L : m->layers) {
        const wrk_buf* vecs[] = {L.ln1_w, L.ln1_b, L.ln2_w, L.ln2_b, L.x_r, L.x_w, L.x_k, L.x_v, L.x_a, L.x_g, L.w0, L.a0, L.v0,
                                 L.r_k, L.k_k, L.k_a, L.gn_w, L.gn_b, L.ffn_x_k};
        for (const wrk_buf* b : vecs) fb(b);
        const wrk_matrix* mats[] = {L.w1, L.w2, L.a1, L.a2, L.g1, L.g2, L.v1, L.v2, L.w_k, L.w_v, L.w_r, L.w_o, L.ffn_w_k, L.ffn_w_v};
        for (const wrk_matrix* x : mats) fm(x);
    }
    delete m;
    return WRK_OK;
}

// A = sum(weight tensors read per token) + 2*L*D*(S+2)*4*B + B*(D*2 + V*4)
size_t wrk_v7_model_token_bytes(const wrk_v7_model* m, uint32_t B) {
    if (!m) return 0;
    const size_t D = m->d.num_emb, S = D / m->d.num_head, V = m->d.num_vocab;
    size_t w = wrk_matrix_stream_bytes(m->head) + 4 * D * 2;     // head + ln0/ln_out vectors
    for (uint32_t l = 0; l < m->d.num_layer; ++l) {
        const wrk_v7_layer_desc& L = m->layers[l];
        const wrk_matrix* mats[] = {L.w1, L.w2, L.a1, L.a2, L.g1, L.g2, L.w_k, L.w_v, L.w_r, L.w_o, L.ffn_w_k, L.ffn_w_v};
        for (const wrk_matrix* x : mats) w += wrk_matrix_stream_bytes(x);
        if (l > 0) w += wrk_matrix_stream_bytes(L.v1) + wrk_matrix_stream_bytes(L.v2) + D * 2;
        w += 18 * D * 2;                                         // f16 vectors of the layer
    }
    return w + 2 * (size_t)m->d.num_layer * D * (S + 2) * 4 * B + (size_t)B * (D * 2 + V * 4);
}

int32_t wrk_v7_state_create(wrk_ctx* ctx, const wrk_v7_model* model, uint32_t num_batch, wrk_v7_state** out) {
    if (!ctx || !model || !out) return WRK_E_ARG;
    LOCK(ctx);
    *out = nullptr;
    WRK_ARG(ctx, num_batch >= 1 && num_batch <= 255, "num_batch must be 1..255 (cursor batch is u8, tensor/mod.rs:53-60)");
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_v7_state* st = new wrk_v7_state();
    st->ctx = ctx;
    st->num_layer = model->d.num_layer;
    st->num_emb = model->d.num_emb;
    st->head_size = model->d.num_emb / model->d.num_head;
    st->num_batch = num_batch;
    const size_t bytes = st->layer_elems() * st->num_layer * 4;
    hipError_t e = hipMalloc((void**)&st->data, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(st->data, 0, bytes, ctx->stream);
    if (e != hipSuccess) { delete st; return wrk_fail(ctx, e == hipErrorOutOfMemory ? WRK_E_OOM : WRK_E_HIP, "state alloc: %s", hipGetErrorString(e)); }
    *out = st;
    return WRK_OK;
}

int32_t wrk_v7_state_destroy(wrk_v7_state* st) {
    if (!st) return WRK_E_ARG;
    {
        LOCK(st->ctx);
        hipSetDevice(st->ctx->device);
        hipStreamSynchronize(st->ctx->stream);
        hipFree(st->data);
    }
    delete st;
    return WRK_OK;
}

// host layout [L][S+2][D] (reference shape [D, S+2, L, 1], x fastest); device [L][B][S+2][D]
int32_t wrk_v7_state_load(wrk_ctx* ctx, wrk_v7_state* st, uint32_t batch, const float* src) {
    if (!ctx || !st || !src) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, batch < st->num_batch, "batch %u out of range", batch);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)(st->head_size + 2) * st->num_emb;
    for (uint32_t l = 0; l < st->num_layer; ++l)
        WRK_HIP(ctx, hipMemcpyAsync(st->layer_ptr(l) + batch * per, src + l * per, per * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_v7_state_back(wrk_ctx* ctx, const wrk_v7_state* st, uint32_t batch, float* dst) {
    if (!ctx || !st || !dst) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, batch < st->num_batch, "batch %u out of range", batch);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t per = (size_t)(st->head_size + 2) * st->num_emb;
    for (uint32_t l = 0; l < st->num_layer; ++l)
        WRK_HIP(ctx, hipMemcpyAsync(dst + l * per, st->layer_ptr(l) + batch * per, per * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

static int32_t state_d2d(wrk_ctx* ctx, const wrk_v7_state* st, uint32_t batch, const wrk_buf* buf, bool to_state) {
    if (!ctx || !st || !buf) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, batch < st->num_batch, "batch %u out of range", batch);
    const size_t per = (size_t)(st->head_size + 2) * st->num_emb;
    WRK_ARG(ctx, buf->bytes >= per * st->num_layer * 4, "snapshot buffer holds %zu bytes, a state needs %zu", buf->bytes, per * st->num_layer * 4);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    for (uint32_t l = 0; l < st->num_layer; ++l) {
        float* slot = st->layer_ptr(l) + batch * per;
        float* snap = (float*)buf->ptr + l * per;
        WRK_HIP(ctx, hipMemcpyAsync(to_state ? slot : snap, to_state ? snap : slot, per * 4, hipMemcpyDeviceToDevice, ctx->op_stream()));
    }
    return WRK_OK;
}

int32_t wrk_v7_state_read(wrk_ctx* ctx, const wrk_v7_state* st, uint32_t batch, wrk_buf* buf) { return state_d2d(ctx, st, batch, buf, false); }
int32_t wrk_v7_state_write(wrk_ctx* ctx, wrk_v7_state* st, uint32_t batch, const wrk_buf* buf) { return state_d2d(ctx, st, batch, buf, true); }

// one RnnJob: wrk_v7_infer, or with a.score wrk_v7_score (the header rows' logits scored against targets instead of read back)
static int32_t v7_job(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const wrk_job_args& a, uint32_t mode) {
    if (!ctx || !m || !st) return WRK_E_ARG;
    LOCK(ctx);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t T = a.T, NH = a.NH, V = m->d.num_vocab;
    if (T == 0) return WRK_OK;                                  // v7.rs:626-635: empty job
    WRK_ARG(ctx, a.cursors, "cursors required");
    WRK_ARG(ctx, a.tokens || a.emb_rows, "either token ids or gathered embedding rows are required");
    WRK_ARG(ctx, !a.tokens || m->emb, "token ids given but the model has no device embedding table");
    WRK_ARG(ctx, NH == 0 || a.headers, "headers required");
    WRK_ARG(ctx, st->num_emb == m->d.num_emb && st->num_layer == m->d.num_layer, "state does not belong to this model");
    wrk_job_shape sh;
    int32_t rc = wrk_job_check(ctx, st, a.cursors, T, a.tokens, V, a.headers, NH, &sh);
    if (rc == WRK_OK) rc = wrk_score_check(ctx, a, V, "wrk_v7_score");
    if (rc == WRK_OK) rc = m->ensure_scratch(T, NH ? NH : 1);
    if (rc == WRK_OK && T == 1 && mode == 1) rc = m->ensure_engine();
    if (rc != WRK_OK) return rc;
    const bool fused = (mode == 1 && sh.one_token_each && sh.nseq == T && m->act_dtype == WRK_F16), want_argmax = NH && a.argmax;
    const uint32_t batch0 = a.cursors[0] & 0xffu;
    rc = wrk_job_upload(*m, m->s, m->s.input, m->emb, m->d.num_emb, a, !fused);
    if (rc != WRK_OK) return rc;
    // The launches of a job depend only on its shape (token count, header rows, flags): cursors, tokens and header rows
    // are device data.  Capture once per shape and replay (the reference caches the RnnJob of a repeated RnnInfo);
    // a 128-token chunk of one sequence is ~1 400 small launches, which replay at graph rate.
    m->wkv_nseq = sh.nseq;    // chunk kernel of the WKV state: one wave or four per head (part of the graph key below)
    auto enqueue_job = [&]() -> int32_t {
        int32_t r;
        if (fused) r = m->enqueue_fused_decode(st, T, NH, sh.identity, a.tokens != nullptr, want_argmax, false, batch0, sh.contiguous);
        else {
            r = m->enqueue_ops(st, T, NH, sh.identity, mode == 1);
            if (r == WRK_OK && want_argmax) wrk::argmax_rows(ctx->op_stream(), m->s.head_o, V, V, NH, m->s.argmax);
        }
        // scoring: the epilogue on head_o, which every path above materialises
        if (r == WRK_OK && a.score && NH &&
            wrk::score_rows(ctx->op_stream(), m->s.head_o, V, V, NH, m->score.targets, m->score.part, m->score.logprob, m->score.rank,
                            ctx->num_cu) != 0)
            r = wrk_fail(ctx, WRK_E_UNSUPPORTED, "score: vocabulary of %u tokens", V);
        return r;
    };
    static const bool no_graph = wrk_no_graph();
    if (no_graph || ctx->capturing_here()) rc = enqueue_job();
    else {
        // bit 5: a non-fused job enqueues the merged launch list in mode 1 and the reference op list in mode 0 -- two graphs
        const uint32_t flags = 16u | (m->act_dtype == WRK_F32 ? 64u : 0u) | (fused ? 1u : 0u) | (sh.identity ? 2u : 0u) | (a.tokens ? 4u : 0u) | (want_argmax ? 8u : 0u) |
                               ((!fused && mode == 1) ? 32u : 0u) | (fused ? batch0 << 8 : 0u) | ((fused && sh.contiguous) ? 1u << 16 : 0u) |
                               ((fused && T == 1 && m->engine_on()) ? 1u << 17 : 0u) | (split_head_env_on() ? 0u : 1u << 18) |
                               ((!fused && (size_t)sh.nseq * m->d.num_head >= 768) ? 1u << 19 : 0u) | (a.score ? 1u << 20 : 0u);
        const wrk_v7_model::GraphKey key{st->uid, T, flags, NH};
        if (!m->graphs.count(key) && m->graphs.size() > 64) { WRK_HIP(ctx, hipStreamSynchronize(ctx->stream)); m->drop_graphs(); }    // bound the cache
        wrk_program* prog = nullptr;
        rc = wrk_cached_program(ctx, m->graphs, key, enqueue_job, &prog);
        if (rc != WRK_OK) return rc;
        WRK_HIP(ctx, hipGraphLaunch(prog->exec, ctx->stream));
    }
    if (rc == WRK_OK) rc = wrk_job_read_back(*m, m->s, V, a);
    if (rc != WRK_OK || ctx->capturing_here()) return rc;
    return wrk_v7_engine_check(m->engine);
}

int32_t wrk_v7_infer(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* tokens, const uint16_t* emb_rows,
                     const uint32_t* cursors, uint32_t T, const uint32_t* headers, uint32_t NH, float* logits, uint32_t* argmax,
                     uint32_t mode) {
    return v7_job(ctx, m, st, {tokens, emb_rows, cursors, T, headers, NH, logits, argmax, false, nullptr, nullptr, nullptr}, mode);
}

int32_t wrk_v7_score(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* tokens, const uint16_t* emb_rows,
                     const uint32_t* cursors, uint32_t T, const uint32_t* headers, uint32_t NH, const uint32_t* targets, float* logprob,
                     uint32_t* rank, uint32_t mode) {
    return v7_job(ctx, m, st, {tokens, emb_rows, cursors, T, headers, NH, nullptr, nullptr, true, targets, logprob, rank}, mode);
}

// Bundle::<F>::new (v7.rs:514-536): the activation type of the frame.  F16 is the reference's default build
// (`Bundle::<f16>`); F32 stores every Runtime<F> buffer in f32 and takes the op-by-op path with f32-input matmuls.
int32_t wrk_v7_model_set_frame_dtype(wrk_ctx* ctx, wrk_v7_model* m, uint32_t dtype) {
    if (!ctx || !m) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, dtype == WRK_F16 || dtype == WRK_F32, "frame dtype must be WRK_F16 or WRK_F32");
    WRK_ARG(ctx, !ctx->capturing_here(), "cannot change the frame inside a capture");
    if (dtype == m->act_dtype) return WRK_OK;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    m->drop_graphs();
    if (m->scratch) hipFree(m->scratch);
    m->scratch = nullptr;
    m->scratch_tokens = m->scratch_headers = 0;
    m->act_dtype = dtype;
    // the concurrent-pipeline lanes carry the frame type they were created with (and programs captured for it): drop them, the next
    // generate_greedy(groups > 1) rebuilds them with the new type
    for (hipStream_t ls : m->lane_streams) WRK_HIP(ctx, hipStreamSynchronize(ls));
    std::vector<wrk_v7_model*> old_lanes;
    old_lanes.swap(m->lanes);
    for (wrk_v7_model* lane : old_lanes) wrk_v7_model_destroy(lane);
    return WRK_OK;
}

int32_t wrk_v7_model_engine_status(wrk_ctx* ctx, wrk_v7_model* m, char* why, size_t capacity) {
    if (!ctx || !m) return WRK_E_ARG;
    LOCK(ctx);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    WRK_ARG(ctx, !ctx->capturing_here(), "not inside a capture");
    const int32_t rc = m->ensure_engine();
    if (rc != WRK_OK) return rc;
    if (why && capacity) {
        // with an engine: how it was built ("8 compute waves"), so that a caller can tell which kernel its tokens run on
        const std::string w = m->engine ? std::to_string(wrk_v7_engine_waves(m->engine)) + " compute waves"
                                        : (m->engine_tried ? m->engine_why : std::string("disabled (WRK_ENGINE=0 or f32 frames)"));
        snprintf(why, capacity, "%s", w.c_str());
    }
    return m->engine ? 1 : 0;
}

// Teacher-forced run of ONE layer (parity tests; the reference reaches the same buffers through v7::HookMap closures over
// `Frame`, v7.rs:386-421, examples/inspect.rs:100-248): the layer's op list (mode 0), or its fused / merged launches (mode 1),
// on a caller-supplied layer input.  Every Runtime<F> buffer of the frame stays readable through wrk_v7_frame_read.
int32_t wrk_v7_infer_layer(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, uint32_t layer, const void* x, const void* v_first,
                           const uint32_t* cursors, uint32_t T, uint32_t mode) {
    if (!ctx || !m || !st || !x || !cursors) return WRK_E_ARG;
    LOCK(ctx);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_v7_infer_layer cannot be captured");
    WRK_ARG(ctx, layer < m->d.num_layer, "layer %u out of range", layer);
    WRK_ARG(ctx, T >= 1, "no tokens");
    WRK_ARG(ctx, layer == 0 || v_first, "layers above 0 read the layer-0 value (att_v0)");
    WRK_ARG(ctx, st->num_emb == m->d.num_emb && st->num_layer == m->d.num_layer, "state does not belong to this model");
    wrk_job_shape sh;
    int32_t rc = wrk_job_check(ctx, st, cursors, T, nullptr, 0, nullptr, 0, &sh);
    if (rc == WRK_OK) rc = m->ensure_scratch(T, 1);
    if (rc == WRK_OK && T == 1 && mode == 1) rc = m->ensure_engine();
    if (rc != WRK_OK) return rc;
    const size_t esz = m->act_dtype == WRK_F32 ? 4 : 2;
    rc = wrk_buf_write_raw(ctx, m->s.cursors, cursors, (size_t)T * 4);
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, m->s.x, x, (size_t)T * m->d.num_emb * esz);
    if (rc == WRK_OK && v_first) rc = wrk_buf_write_raw(ctx, m->s.att_v0, v_first, (size_t)T * m->d.num_emb * esz);
    if (rc != WRK_OK) return rc;
    m->layer_begin = layer; m->layer_end = layer + 1; m->skip_embed = true;
    m->wkv_nseq = sh.nseq;
    // this entry point exists to read the frame buffers of a layer back (wrk_v7_frame_read): the engine keeps them in LDS and granules,
    // so the launches run here; WRK_ENGINE_INSPECT=1 (tests/test_gpu_engine.py) runs the engine's layer instead
    { const char* ei = getenv("WRK_ENGINE_INSPECT"); m->engine_skip_once = !(ei && ei[0] == '1'); }
    if (mode == 1 && sh.one_token_each && sh.nseq == T && m->act_dtype == WRK_F16) rc = m->enqueue_fused_decode(st, T, 0, true, false, false, false, cursors[0] & 0xff, sh.contiguous);
    else rc = m->enqueue_ops(st, T, 0, true, mode == 1);
    m->layer_begin = 0; m->layer_end = 0xffffffffu; m->skip_embed = false; m->engine_skip_once = false;
    if (rc != WRK_OK) return rc;
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return wrk_v7_engine_check(m->engine);
}

// TensorGpu::back on one buffer of the frame (names as examples/inspect.rs:208-248: x, att_x, att_r, ..., ffn_v; plus head_x, head_o)
int32_t wrk_v7_frame_read(wrk_ctx* ctx, wrk_v7_model* m, const char* name, uint32_t T, void* dst, size_t capacity, size_t* bytes) {
    if (!ctx || !m || !name || !bytes) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, m->scratch && T >= 1 && T <= m->scratch_tokens, "no frame of %u tokens has been run", T);
    const uint32_t D = m->d.num_emb, F = m->d.num_hidden;
    const V7Scratch& s = m->s;
    struct { const char* n; const void* p; uint32_t c; } tab[] = {
        {"x", s.x, D}, {"att_x", s.att_x, D}, {"att_v0", s.att_v0, D}, {"att_rx", s.rx, D}, {"att_wx", s.wx, D}, {"att_kx", s.kx, D},
        {"att_vx", s.vx, D}, {"att_ax", s.ax, D}, {"att_gx", s.gx, D}, {"att_r", s.r, D}, {"att_w", s.w, D}, {"att_k", s.k, D}, {"att_v", s.v, D},
        {"att_a", s.a, D}, {"att_g", s.g, D}, {"att_o", s.o, D}, {"att_kk", s.kk, D}, {"att_vv", s.vv, D}, {"att_n", s.n, 4 * D},
        {"aux_w", s.aux_w, m->d.lora_w}, {"aux_a", s.aux_a, m->d.lora_a}, {"aux_g", s.aux_g, m->d.lora_g}, {"aux_v", s.aux_v, m->d.lora_v},
        {"ffn_x", s.ffn_x, D}, {"ffn_kx", s.ffn_kx, D}, {"ffn_k", s.ffn_k, F}, {"ffn_v", s.ffn_v, D}, {"att_x_ln", s.ln_tmp, D}};
    const size_t esz = m->act_dtype == WRK_F32 ? 4 : 2;
    for (auto& e : tab)
        if (strcmp(e.n, name) == 0) {
            const size_t n = (size_t)e.c * T * esz;
            *bytes = n;
            if (!dst) return WRK_OK;
            WRK_ARG(ctx, capacity >= n, "frame buffer %s needs %zu bytes, capacity %zu", name, n, capacity);
            WRK_HIP(ctx, hipSetDevice(ctx->device));
            WRK_HIP(ctx, hipMemcpyAsync(dst, e.p, n, hipMemcpyDeviceToHost, ctx->stream));
            WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return WRK_OK;
        }
    return wrk_fail(ctx, WRK_E_ARG, "no frame buffer named %s", name);
}

}  // extern "C"

// one decode step of sequences [b0, b0 + B) on this frame: embed s.tokens, run the layers and the head, then wrk_enqueue_pick.  The fused
// greedy head leaves the arg-max in s.argmax, and in a plain step advances tokens / history / counter itself: nothing follows it.  A
// constrained, a DRY, a biased or a guided step picks on the modified row, and a beam step makes no pick: its head only writes head_o, as a sampled step's does
int32_t wrk_v7_model::enqueue_step(wrk_v7_state* st, uint32_t b0, uint32_t B, uint32_t mode, wrk_step_kind kind) {
    int32_t rc;
    const bool fused = mode == 1 && act_dtype == WRK_F16, head_picks = fused && !kind.sampled() && !kind.constrained && !kind.dry && !kind.biased && !kind.guided && kind.tail != wrk_step_kind::BEAM,
               head_advances = head_picks && kind.tail == wrk_step_kind::PLAIN && !kind.logprobs;     // log-probs go between the pick and the advance
    if (fused) rc = enqueue_fused_decode(st, B, B, true, true, head_picks, head_advances, b0, true);
    else {
        wrk::gather_rows_f16(ctx->op_stream(), emb->ptr, s.tokens, s.input, d.num_emb, B);
        rc = enqueue_ops(st, B, B, true);
    }
    if (rc != WRK_OK || head_advances) return rc;
    return wrk_enqueue_pick(*this, B, kind, st, b0, head_picks);
}

int32_t wrk_v7_model::ensure_frame(uint32_t B, uint32_t mode) {
    const int32_t rc = ensure_scratch(B, B);
    return rc == WRK_OK && B == 1 && mode == 1 ? ensure_engine() : rc;
}

// mode, f32 frames (4), the engine (8), the unsplit head (16)
uint32_t wrk_v7_model::key_bits(uint32_t B, uint32_t mode) const {
    return mode | (act_dtype == WRK_F32 ? 4u : 0u) | ((B == 1 && mode == 1 && engine_on()) ? 8u : 0u) | (split_head_env_on() ? 0u : 16u);
}

// lane 0 is this model's own frame; lanes 1.. are clones sharing the weight handles, created with their streams and events on demand
int32_t wrk_v7_model::lane(uint32_t g, uint32_t groups, wrk_frame_common** out) {
    while (lanes.size() + 1 < groups) {
        wrk_v7_model* clone = nullptr;
        const int32_t rc = wrk_v7_model_create(ctx, &d, &clone);
        if (rc != WRK_OK) return rc;
        clone->act_dtype = act_dtype;
        lanes.push_back(clone);
    }
    while (lane_streams.size() < groups) {
        hipStream_t ls = nullptr;
        hipEvent_t e = nullptr;
        WRK_HIP(ctx, hipStreamCreateWithFlags(&ls, hipStreamNonBlocking));
        WRK_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        lane_streams.push_back(ls);
        lane_events.push_back(e);
    }
    wrk_v7_model* mdl = g == 0 ? this : lanes[g - 1];
    // the persistent engine needs every CU for itself: two of them side by side (one per lane) would each hold part of the chip
    // and wait for the rest forever (until their bounded spins give up) -- concurrent pipelines keep the five-launch layer
    mdl->engine_blocked = groups > 1;
    *out = mdl;
    return WRK_OK;
}

void wrk_v7_model::before_loop() { wrk::timing_slot(ctx, nullptr); }     // WRK_TIMING=1: allocate the stamp buffer outside the capture

int32_t wrk_v7_model::after_loop(uint32_t groups) {
    wrk::timing_report(ctx);
    for (uint32_t g = 0; g < groups; ++g) {
        wrk_v7_engine* e = (g == 0 ? this : lanes[g - 1])->engine;
        wrk_v7_engine_report(e);
        const int32_t rc = wrk_v7_engine_check(e);
        if (rc != WRK_OK) return rc;
    }
    return WRK_OK;
}

extern "C" {

int32_t wrk_v7_generate_greedy(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B,
                               uint32_t steps, uint32_t* out_tokens, float* last_logits, float* elapsed_ms, uint32_t mode_arg) {
    return wrk_generate(ctx, m, st, first_tokens, B, steps, wrk_pick_args{}, out_tokens, last_logits, elapsed_ms, mode_arg);
}

int32_t wrk_v7_generate_sample(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B, uint32_t steps,
                               const float* temperature, const float* top_p, const uint32_t* seed, uint32_t* out_tokens, float* last_logits,
                               float* elapsed_ms, uint32_t mode_arg) {
    wrk_pick_args pick{temperature, top_p, seed};
    pick.need = wrk_pick_args::SAMPLER;
    return wrk_generate(ctx, m, st, first_tokens, B, steps, pick, out_tokens, last_logits, elapsed_ms, mode_arg);
}

int32_t wrk_v7_generate_penalized(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B, uint32_t steps,
                                  const float* temperature, const float* top_p, const uint32_t* seed, const float* presence,
                                  const float* frequency, const float* decay, wrk_occurrence* occ, uint32_t* out_tokens, float* last_logits,
                                  float* elapsed_ms, uint32_t mode_arg) {
    wrk_pick_args pick{temperature, top_p, seed, presence, frequency, decay, occ};
    pick.need = wrk_pick_args::TABLE;
    return wrk_generate(ctx, m, st, first_tokens, B, steps, pick, out_tokens, last_logits, elapsed_ms, mode_arg);
}

int32_t wrk_v7_generate_stop(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B, uint32_t steps,
                             const wrk_generate_options* opt, uint32_t* out_tokens, uint32_t* out_lengths, float* last_logits,
                             uint32_t* steps_run, float* elapsed_ms, uint32_t mode_arg) {
    const wrk_stop_call stop{opt, out_lengths, steps_run};
    return wrk_generate(ctx, m, st, first_tokens, B, steps, opt ? wrk_pick_of(*opt) : wrk_pick_args{}, out_tokens, last_logits, elapsed_ms, mode_arg, &stop);
}

int32_t wrk_v7_generate_queue(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                              const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg) {
    return wrk_generate_queue(ctx, m, st, B, opt, out_arg, elapsed_ms, mode_arg, wrk_step_kind::QUEUE, nullptr);
}

int32_t wrk_v7_generate_queue_pool(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                                   const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, const wrk_queue_pool* pool) {
    return wrk_generate_queue(ctx, m, st, B, opt, out_arg, elapsed_ms, mode_arg, wrk_step_kind::QUEUE_POOL, pool);
}

int32_t wrk_v7_generate_queue_guided(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                                     const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, const wrk_queue_guidance* guide) {
    return wrk_generate_queue(ctx, m, st, B, opt, out_arg, elapsed_ms, mode_arg, wrk_step_kind::QUEUE, nullptr, guide, true);
}

int32_t wrk_v7_generate_queue_cut(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                                  const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, const wrk_queue_cuts* cuts) {
    return wrk_generate_queue_cut(ctx, m, st, B, opt, out_arg, elapsed_ms, mode_arg, cuts);
}

int32_t wrk_v7_generate_beam(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t G, uint32_t steps,
                             const wrk_beam_options* opt, const wrk_beam_result* out_arg, float* elapsed_ms, uint32_t mode_arg) {
    return wrk_generate_beam(ctx, m, st, first_tokens, G, steps, opt, out_arg, elapsed_ms, mode_arg);
}

int32_t wrk_v7_generate_beam_context(wrk_ctx* ctx, wrk_v7_model* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t G, uint32_t steps,
                                     const wrk_beam_options* opt, const wrk_beam_result* out_arg, float* elapsed_ms, uint32_t mode_arg,
                                     const wrk_beam_context* bc) {
    return wrk_generate_beam(ctx, m, st, first_tokens, G, steps, opt, out_arg, elapsed_ms, mode_arg, bc);
}

}  // extern "C"

// Persistent decode engine: built once, outside captures.  WRK_ENGINE=0 keeps the five-launch layer (read per call, part of the
// graph key: tests compare the two paths in one process).
static bool engine_env_on() { const char* e = getenv("WRK_ENGINE"); return !(e && e[0] == '0'); }
bool engine_env_on_public() { return engine_env_on(); }
bool wrk_v7_model::engine_on() const { return engine != nullptr && !engine_blocked && engine_env_on() && act_dtype == WRK_F16; }
int32_t wrk_v7_model::ensure_engine() {
    if (engine_tried || !engine_env_on() || act_dtype != WRK_F16) return WRK_OK;
    if (ctx->capturing_here()) return WRK_OK;       // allocations are not capturable: the caller's program keeps the launches
    engine_tried = true;
    const std::string keep = ctx->err;
    const int32_t rc = wrk_v7_engine_create(this, &engine);
    if (rc != WRK_OK) { engine = nullptr; engine_why = ctx->err; ctx->err = keep; }
    if (rc != WRK_OK && rc != WRK_E_UNSUPPORTED) return rc;
    return WRK_OK;
}
