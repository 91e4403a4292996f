// Internal definitions of the RWKV-7 model handle: its frame layout, the concurrent-pipeline lanes and the decode engine.  The state
// handle and everything the RWKV-6 runner shares with this one live in wrk_runner.h.
#pragma once
#include <string>
#include <vector>

#include "wrk_runner.h"

struct V7Scratch : wrk::FrameIo {      // Runtime<f16> + Header<f16> (v7.rs:281-383); f16 unless noted; head_o: f32 [V, num_header]
    void *input, *x, *att_x, *att_v0, *rx, *wx, *kx, *vx, *ax, *gx, *r, *w, *k, *v, *a, *g, *o, *kk, *vv, *n;
    void *aux_w, *aux_a, *aux_g, *aux_v, *ffn_x, *ffn_kx, *ffn_k, *ffn_v, *ln_tmp, *head_x;
    float* ks_part; uint32_t* ks_cnt; size_t ks_part_cap; uint32_t ks_cnt_cap;     // K-sliced GEMM scratch (2 .. 64 tokens), see MatJob
};

struct wrk_v7_model : wrk_frame_common {
    wrk_v7_model_desc d{};
    std::vector<wrk_v7_layer_desc> layers;
    const wrk_buf *ln0_w = nullptr, *ln0_b = nullptr, *ln_out_w = nullptr, *ln_out_b = nullptr, *emb = nullptr;
    const wrk_matrix* head = nullptr;

    V7Scratch s{};

    // fused decode path (wrk_v7_fused.hip): arg-max partials of the head matvec [num_wg][num_header]
    float* amax_val = nullptr;
    uint32_t* amax_idx = nullptr;
    size_t amax_cap = 0;

    // teacher-forced single-layer runs (wrk_v7_infer_layer): the layer range the op list covers and whether the embedding
    // stage (LN(ln0) + blit) is part of it; the defaults are the whole model
    uint32_t layer_begin = 0, layer_end = 0xffffffffu;
    bool skip_embed = false;
    // activation dtype of the frame: WRK_F16 = Bundle::<f16> (the reference's default), WRK_F32 = Bundle::<f32> (v7.rs:281-320
    // is generic over F).  F32 frames always take the op-by-op path with the f32-input matvec.
    uint32_t act_dtype = WRK_F16;

    // Concurrent pipelines (generate_greedy with groups > 1): lane g is a clone of this model -- same weight handles, its own frame,
    // history and cached programs -- whose decode graphs are replayed on a stream of its own, so that several latency-bound
    // pipelines overlap on the GPU (independent sequences: separate state slices, no synchronisation between lanes)
    std::vector<wrk_v7_model*> lanes;

    // persistent batch-1 decode engine (wrk_v7_engine.hip): built on first use, nullptr when the model / device does not fit it
    struct wrk_v7_engine* engine = nullptr;
    bool engine_tried = false;
    bool engine_skip_once = false;      // wrk_v7_infer_layer: the frame buffers must be materialised -> launches (unless WRK_ENGINE_INSPECT=1)
    bool engine_blocked = false;        // set by lane() while several pipelines share the GPU (groups > 1), cleared by the next call on one
    std::string engine_why;             // why the engine is not available (diagnostics)
    int32_t ensure_engine();            // outside captures; WRK_OK also when the engine is unavailable
    bool engine_on() const;             // WRK_ENGINE != 0 and the engine exists
    // the runner interface of the decode loops (wrk_runner.h)
    Facts facts() const override { return {d.num_vocab, d.num_emb, d.num_layer, emb != nullptr}; }
    wrk::FrameIo& io() override { return s; }
    int32_t ensure_frame(uint32_t B, uint32_t mode) override;
    int32_t enqueue_step(wrk_v7_state* st, uint32_t b0, uint32_t B, uint32_t mode, wrk_step_kind kind) override;
    uint32_t key_bits(uint32_t B, uint32_t mode) const override;
    uint32_t max_lanes() const override { return 255; }
    int32_t lane(uint32_t g, uint32_t groups, wrk_frame_common** out) override;
    void before_loop() override;
    int32_t after_loop(uint32_t groups) override;
    int32_t ensure_scratch(uint32_t T, uint32_t NH);
    int32_t enqueue_ops(wrk_v7_state* st, uint32_t T, uint32_t NH, bool identity_headers, bool merged = false);
    // from_tokens: gather embedding rows of s.tokens on the device; want_argmax: greedy token per header row into
    // s.argmax; advance: also feed it back as the next token (device-resident generation loop)
    int32_t enqueue_fused_decode(wrk_v7_state* st, uint32_t B, uint32_t NH, bool identity_headers, bool from_tokens,
                                 bool want_argmax, bool advance, uint32_t cursor0_batch, bool contiguous);   // batch id of token 0; contiguous: token t is batch cursor0_batch + t
    void free_fused();
};

bool split_head_env_on();     // WRK_SPLIT_HEAD != 0, read per call (part of the graph keys)
bool engine_env_on_public();  // WRK_ENGINE != 0, read per call
