/*
 * wrk_hip.h -- C ABI of the MI355X (gfx950) backend for the RWKV hot path of
 * JoelTankard/web-rwkv-gguf.
 *
 * This is the drop-in boundary described in SURVEY.md section 8(b): everything the reference's
 * `Context` (src/context.rs) does through wgpu for the model path -- allocate/upload/read back
 * buffers, build a TensorOp, encode a list of ops, submit -- has one entry point here.  The
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an int32_t status (WRK_OK == 0); out-params come last;
 *     nothing unwinds across the boundary; `wrk_last_error(ctx)` returns the message.
 *   - plain pointers and sizes only; host pointers are borrowed for the duration of the call.
 *   - handles are reference counted where the reference uses Arc<Buffer>.
 *   - tensors are `[x = fastest, y, z, w]` exactly like src/tensor/shape.rs:95-99 and are
 *     addressed through `wrk_view` == `View { shape, stride, offset }` (src/tensor/mod.rs:27-44):
 *     element(b, t, c) = ((b + offset[2]) * stride[1] + (t + offset[1])) * stride[0] + c + offset[0]
 *     (`stride` holds the parent tensor's dims, as in the WGSL `compute_index` helpers).
 *   - `wrk_op_*` functions ENQUEUE work on the context's submission stream (they are the HIP analogue of
 *     building a TensorOp and encoding it); between `wrk_capture_begin/end` ON THE SAME THREAD they are
 *     recorded into a `wrk_program` (a hipGraph) instead, which is the analogue of the CommandBuffer the
 *     reference keeps in an `RnnJob` (src/runtime/v7.rs:423-432) and replays with `queue.submit`.
 *   - threading = the reference's: jobs are ENCODED concurrently on tokio `spawn_blocking` workers
 *     while the runtime task SUBMITS cached ones (src/runtime/mod.rs:139-167) and a dedicated thread blocks in
 *     read-backs (src/context.rs:148-162).  A capture belongs to the thread that began it and records on a
 *     private stream: the submission stream and the read-back stream are never in capture mode, any number of
 *     threads may have a capture open, and launches / uploads / allocations / reads from other threads proceed
 *     meanwhile.  Individual calls on one context are serialised by an internal mutex (a capture is not).
 *     Nothing recorded executes before its program is launched; `wrk_buf_write` is never recorded (it is
 *     `queue.write_buffer`, not an encoder command); `wrk_buf_copy` and the state snapshot copies are.
 */
#ifndef WRK_HIP_H
#define WRK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WRK_ABI_VERSION 1

typedef struct wrk_ctx wrk_ctx;         /* Context              src/context.rs:51-64        */
typedef struct wrk_buf wrk_buf;         /* Arc<Buffer>          src/context.rs:368-394      */
typedef struct wrk_matrix wrk_matrix;   /* enum Matrix          src/tensor/matrix.rs:82-131 */
typedef struct wrk_program wrk_program; /* Vec<CommandBuffer>   src/tensor/ops.rs:79-143    */
typedef struct wrk_v7_model wrk_v7_model; /* v7::Model          src/runtime/v7.rs:35-142    */
typedef struct wrk_v7_state wrk_v7_state; /* v7::State          src/runtime/v7.rs:146-277   */

enum {
    WRK_OK = 0,
    WRK_E_ARG = 1,          /* TensorError::{Shape,Size,Type,...}                      */
    WRK_E_OOM = 2,
    WRK_E_HIP = 3,          /* ContextError / device lost                              */
    WRK_E_UNSUPPORTED = 4
};

enum { WRK_F16 = 0, WRK_F32 = 1, WRK_U8 = 2, WRK_U32 = 3 };

/* Activation (src/tensor/ops.rs:146-160, definitions :205-235) */
enum {
    WRK_ACT_NONE = 0,
    WRK_ACT_SQUARED_RELU = 1,
    WRK_ACT_TANH = 2,
    WRK_ACT_STABLE_EXP = 3,
    WRK_ACT_OPPOSITE_EXP = 4,
    WRK_ACT_SOFTPLUS = 5,
    WRK_ACT_SIGMOID = 6,
    WRK_ACT_SILU = 7
};

/* Matrix variants (src/tensor/matrix.rs:82-131).  Values of the GGUF kinds equal the ggml type
 * ids (src/runtime/gguf.rs:888-923) so a loader can pass `info.tensor_type` through. */
enum {
    WRK_MAT_F32 = 0,        /* converted to f16 on upload (loader.rs:117-121)           */
    WRK_MAT_F16 = 1,
    WRK_MAT_Q8_0 = 8,
    WRK_MAT_Q4_K = 12,
    WRK_MAT_Q5_K = 13,
    WRK_MAT_Q6_K = 14,
    WRK_MAT_INT8 = 100,     /* web-rwkv Int8: u8 + per-128 (min,max) f16                 */
    WRK_MAT_NF4 = 101       /* web-rwkv NF4 : u4 + per-64 absmax f16 + 16-entry table    */
};

/* wrk_matrix_create flags */
enum {
    WRK_MATRIX_EXACT = 0,        /* ggml-canonical inline dequantisation in f32 (north_star)          */
    WRK_MATRIX_ROUND_F16 = 1     /* reproduce the reference at HEAD: every dequantised weight is
                                    rounded to f16 first (gguf.rs:129,135)               */
};

typedef struct wrk_view {
    uint32_t shape[4];
    uint32_t stride[4];
    uint32_t offset[4];
} wrk_view;

typedef struct wrk_tensor {     /* TensorGpuView: buffer + dtype + view */
    wrk_buf* buf;
    uint32_t dtype;             /* WRK_F16 / WRK_F32 */
    wrk_view view;
} wrk_tensor;

/* ---------------------------------------------------------------- context (src/context.rs) */
int32_t wrk_abi_version(void);
/* ContextBuilder::build (context.rs:113-165) */
int32_t wrk_ctx_create(int32_t device, wrk_ctx** out);
/* Drop for Context (context.rs:66-78) */
int32_t wrk_ctx_destroy(wrk_ctx* ctx);
const char* wrk_last_error(wrk_ctx* ctx);
/* device.poll(Wait) (context.rs:439-470, v7.rs:1076-1080) */
int32_t wrk_ctx_sync(wrk_ctx* ctx);
/* the HIP stream ops are enqueued on (for callers that time with events or interoperate) */
void* wrk_ctx_stream(wrk_ctx* ctx);

/* ---------------------------------------------------------------- buffers */
/* checkout_buffer(_init) (context.rs:368-394), TensorGpu::from_data_u8 (tensor/mod.rs:603-626) */
int32_t wrk_buf_create(wrk_ctx* ctx, size_t bytes, const void* init_or_null, wrk_buf** out);
int32_t wrk_buf_retain(wrk_buf* buf);
int32_t wrk_buf_release(wrk_buf* buf);                     /* TensorGpu::destroy (tensor/mod.rs:797) */
size_t wrk_buf_size(const wrk_buf* buf);
void* wrk_buf_device_ptr(const wrk_buf* buf);
/* TensorGpu::load / load_batch -> queue.write_buffer (tensor/mod.rs:774-795); stream ordered,
 * the source is copied before the call returns */
int32_t wrk_buf_write(wrk_ctx* ctx, wrk_buf* buf, size_t offset, const void* src, size_t bytes);
/* TensorGpu::back / read_back_buffer (tensor/mod.rs:671-714, context.rs:439-470); blocking */
int32_t wrk_buf_read(wrk_ctx* ctx, const wrk_buf* buf, size_t offset, void* dst, size_t bytes);
/* copy_tensor(_batch) (tensor/ops.rs:35-75) */
int32_t wrk_buf_copy(wrk_ctx* ctx, const wrk_buf* src, size_t src_off, wrk_buf* dst, size_t dst_off, size_t bytes);

/* ---------------------------------------------------------------- programs (encode / submit) */
/* Context::encode (ops.rs:79-143): ops enqueued between begin/end are recorded, not run */
int32_t wrk_capture_begin(wrk_ctx* ctx);
int32_t wrk_capture_end(wrk_ctx* ctx, wrk_program** out);
/* queue.submit(commands) (v7.rs:476-479) */
int32_t wrk_program_launch(wrk_ctx* ctx, wrk_program* prog);
int32_t wrk_program_destroy(wrk_program* prog);

/* ---------------------------------------------------------------- matrices */
/* Loader::load_matrix / try_load_matrix_direct / load_matrix_f16 (loader.rs:617-641,756-921).
 * `data` is the raw GGUF block stream (row-major, rows of K elements, M rows) for the GGUF
 * kinds, or row-major f16/f32 values.  Blocks are re-laid-out on upload;
 * no bytes are added to the weight stream beyond 16-byte row alignment. */
int32_t wrk_matrix_create(wrk_ctx* ctx, uint32_t kind, uint32_t k, uint32_t m,
                          const void* data, size_t bytes, uint32_t flags, wrk_matrix** out);
/* web-rwkv's own formats through wrk_matrix_create (Matrix::Int8 { w, m } / Matrix::Fp4 { w, q, m },
 * matrix.rs:79-130; the direct-load arms loader.rs:808-820, 901-918):
 *   WRK_MAT_INT8: data = u8 codes [K*M] ++ (min, max) f16 pairs, one per 128 flattened elements; K % 16 == 0, K*M % 128 == 0
 *   WRK_MAT_NF4 : data = nibbles [K*M/2] (element 2i in the low nibble) ++ absmax f16, one per 64 flattened
 *                 elements, optionally ++ the 16 f32 levels of `q` (default: the NF4 levels matrix.rs:50-67;
 *                 pass Float4Quant::new_student's for SF4); K % 64 == 0
 *
 * Matrix::quant_u8 / quant_nf4 / quant_sf4 (matrix.rs:211-271; quant_mat_int8.wgsl, quant_mat_nf4.wgsl):
 * on-device quantisation of an f16 [K, M] tensor (`f16_data`: M rows of K values).  `levels`: NULL for the
 * NF4 levels, else 16 f32 (SF4); ignored for WRK_MAT_INT8. */
int32_t wrk_matrix_quantize(wrk_ctx* ctx, uint32_t kind, uint32_t k, uint32_t m,
                            const wrk_buf* f16_data, const float* levels, wrk_matrix** out);
/* read the quantised planes back in wrk_matrix_create's layout (tests; Matrix serialisation): INT8 / NF4 only */
int32_t wrk_matrix_export(wrk_matrix* mat, void* dst, size_t capacity, size_t* bytes);
/* Loader::load_matrix_discount (loader.rs:923-951): the reference multiplies every weight by 2^-(layer / rescale) at load,
 * which forces the F16 path.  A power-of-two factor commutes with the contraction, so the blocks stay quantised and the
 * factor is applied to the f32 dot product instead: y = act(scale * (W . x)). */
int32_t wrk_matrix_set_scale(wrk_matrix* mat, float scale);
int32_t wrk_matrix_release(wrk_matrix* mat);
/* stored bytes read per full pass over the matrix (the roofline's algorithmic bytes) */
size_t wrk_matrix_stream_bytes(const wrk_matrix* mat);

/* ---------------------------------------------------------------- TensorOp constructors
 * One function per reference op on the V7/V6 path.  Shapes are validated as the
 * reference does (TensorError -> WRK_E_ARG). */

/* Matrix::matmul_op (matrix.rs:185-209): output[M, T, B] = act(W[K, M] . input[K, T, B]).
 * turbo != 0 selects the MFMA GEMM kernels for >= 2 stacked tokens (the reference takes T % 32 == 0 there; here token
 * tiles are padded, so any count works); sparse = matmul_op_sparse */
int32_t wrk_op_matmul(wrk_ctx* ctx, const wrk_matrix* mat, const wrk_tensor* input, const wrk_tensor* output,
                      uint32_t act, int32_t turbo, int32_t sparse);
/* TensorOp::layer_norm (ops.rs:407-454): x[C, T, B] in place, w/b f16 [C] */
int32_t wrk_op_layer_norm(wrk_ctx* ctx, const wrk_buf* w, const wrk_buf* b, const wrk_tensor* x, float eps);
/* TensorOp::group_norm (ops.rs:460-508): x[S, H, T], w/b f16 [S*H] */
int32_t wrk_op_group_norm(wrk_ctx* ctx, const wrk_buf* w, const wrk_buf* b, const wrk_tensor* x, float eps);
/* TensorOp::l2_norm (ops.rs:642-691): x[S, H, T] */
int32_t wrk_op_l2_norm(wrk_ctx* ctx, const wrk_tensor* x, float eps);
/* TensorOp::token_shift (ops.rs:2119-2187): cursors u32 [T]; time_mix [C, 1 or T, I] (one factor vector, or V6's
 * per-token factors, I shifts per call); state f32 view [C, 1, B]; input [C, T, 1]; output [C, T, I] */
int32_t wrk_op_token_shift(wrk_ctx* ctx, const wrk_buf* cursors, const wrk_tensor* time_mix, const wrk_tensor* state,
                           const wrk_tensor* input, const wrk_tensor* output, int32_t reversed);
/* TensorOp::transpose (ops.rs:2847-2905): output[C, B, T] = input[C, T, B] */
int32_t wrk_op_transpose(wrk_ctx* ctx, const wrk_tensor* input, const wrk_tensor* output);
/* TensorOp::time_mix_v6 (ops.rs:2327-2394): time_decay/k/v/r/x [S, H, T]; time_first f32 [S*H]; state f32 view [C, S+1, B] */
int32_t wrk_op_time_mix_v6(wrk_ctx* ctx, const wrk_buf* cursors, const wrk_tensor* time_decay, const wrk_buf* time_first,
                           const wrk_tensor* state, const wrk_tensor* k, const wrk_tensor* v, const wrk_tensor* r, const wrk_tensor* x);
/* TensorOp::channel_mix (ops.rs:2586-2641, V6): x <- sigmoid(r) * v, plus the ffn shift-state save */
int32_t wrk_op_channel_mix(wrk_ctx* ctx, const wrk_buf* cursors, const wrk_tensor* state, const wrk_tensor* r, const wrk_tensor* v, const wrk_tensor* x);
/* TensorOp::add_activate / mul_activate (ops.rs:1953-2117): output = act_o(act_x(input) (+|*) act_y(output)),
 * input broadcast over T/B when its extent is 1 */
int32_t wrk_op_add(wrk_ctx* ctx, const wrk_tensor* input, const wrk_tensor* output, uint32_t act_x, uint32_t act_y, uint32_t act_o);
int32_t wrk_op_mul(wrk_ctx* ctx, const wrk_tensor* input, const wrk_tensor* output, uint32_t act_x, uint32_t act_y, uint32_t act_o);
/* TensorOp::lerp (ops.rs:3010-3076): y <- reversed ? mix(y, x, f) : mix(x, y, f) */
int32_t wrk_op_lerp(wrk_ctx* ctx, const wrk_tensor* x, const wrk_tensor* y, const wrk_tensor* f, int32_t reversed);
/* TensorOp::blit (ops.rs:2741-2793): strided copy with dtype conversion */
int32_t wrk_op_blit(wrk_ctx* ctx, const wrk_tensor* input, const wrk_tensor* output);
/* TensorOp::affine (ops.rs:3078-3117): x <- scale * x + bias */
int32_t wrk_op_affine(wrk_ctx* ctx, const wrk_tensor* x, float scale, float bias);
/* TensorOp::activate (ops.rs:2699-2739) */
int32_t wrk_op_activate(wrk_ctx* ctx, const wrk_tensor* x, uint32_t act);
/* TensorOp::control_k_v7 (ops.rs:2526-2584): k <- k * (1 + (a - 1) * p), p f16 [C] */
int32_t wrk_op_control_k_v7(wrk_ctx* ctx, const wrk_buf* p, const wrk_tensor* a, const wrk_tensor* k);
/* TensorOp::time_mix_v7 (ops.rs:2405-2467): state f32 view [C, S+1, B]; r, w, x [S, H, T];
 * n [S, H, T, 4] = (k, v, a, kk) */
int32_t wrk_op_time_mix_v7(wrk_ctx* ctx, const wrk_buf* cursors, const wrk_tensor* state, const wrk_tensor* r,
                           const wrk_tensor* w, const wrk_tensor* n, const wrk_tensor* x);
/* TensorOp::time_first_v7 (ops.rs:2469-2524): u f16 [S, H] */
int32_t wrk_op_time_first_v7(wrk_ctx* ctx, const wrk_buf* u, const wrk_tensor* r, const wrk_tensor* n, const wrk_tensor* x);
/* TensorOp::channel_mix_v7 (ops.rs:2643-2697): state f32 view [C, 1, B]; v, x [C, T] */
int32_t wrk_op_channel_mix_v7(wrk_ctx* ctx, const wrk_buf* cursors, const wrk_tensor* state, const wrk_tensor* v, const wrk_tensor* x);
/* TensorOp::softmax (ops.rs:300-344) -- "next" row (f)1 */
int32_t wrk_op_softmax(wrk_ctx* ctx, const wrk_tensor* x);

/* ---------------------------------------------------------------- fused RWKV-7 fast path
 * New entry points (no reference counterpart at this granularity): they run what
 * v7::Bundle::dispatch (v7.rs:598-713) encodes for one chunk, with the elementwise ops fused
 * into the producing kernels.  Results follow the same rounding points as the op-by-op path. */

typedef struct wrk_v7_layer_desc {
    /* f16 vectors [D] unless noted; v7.rs:77-128 */
    const wrk_buf *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    const wrk_buf *x_r, *x_w, *x_k, *x_v, *x_a, *x_g;
    const wrk_buf *w0, *a0, *v0;
    const wrk_matrix *w1, *w2, *a1, *a2, *g1, *g2, *v1, *v2;     /* v1/v2/v0 unused on layer 0 */
    const wrk_buf *r_k, *k_k, *k_a;
    const wrk_matrix *w_k, *w_v, *w_r, *w_o;
    const wrk_buf *gn_w, *gn_b;
    const wrk_buf* ffn_x_k;
    const wrk_matrix *ffn_w_k, *ffn_w_v;
} wrk_v7_layer_desc;

typedef struct wrk_v7_model_desc {
    uint32_t num_layer, num_emb, num_hidden, num_vocab, num_head;
    uint32_t lora_w, lora_a, lora_g, lora_v;          /* v7::CustomInfo (v7.rs:54-60) */
    uint32_t rescale;                                 /* Model::rescale, default 1024 (v7.rs:50) */
    const wrk_buf *ln0_w, *ln0_b, *ln_out_w, *ln_out_b;
    const wrk_buf* emb_f16;                           /* [D, V] f16 table on device, or NULL when the
                                                         caller gathers rows itself (v7.rs:438-474) */
    const wrk_matrix* head;
    const wrk_v7_layer_desc* layers;
} wrk_v7_model_desc;

/* ModelBuilder::build_v7 after the tensors are uploaded (v7.rs:1038-1227); retains every handle */
int32_t wrk_v7_model_create(wrk_ctx* ctx, const wrk_v7_model_desc* desc, wrk_v7_model** out);
int32_t wrk_v7_model_destroy(wrk_v7_model* model);
/* algorithmic bytes read+written per decoded token for `num_batch` sequences */
size_t wrk_v7_model_token_bytes(const wrk_v7_model* model, uint32_t num_batch);

/* v7::Bundle::new state allocation (v7.rs:514-536): L tensors f32 [D, S+2, B], zeroed */
int32_t wrk_v7_state_create(wrk_ctx* ctx, const wrk_v7_model* model, uint32_t num_batch, wrk_v7_state** out);
int32_t wrk_v7_state_destroy(wrk_v7_state* state);
/* State::load / State::back (v7.rs:152-170, 210-217): host f32 [D, S+2, L] for one batch */
int32_t wrk_v7_state_load(wrk_ctx* ctx, wrk_v7_state* state, uint32_t batch, const float* src);
int32_t wrk_v7_state_back(wrk_ctx* ctx, const wrk_v7_state* state, uint32_t batch, float* dst);
/* State::read / State::write (v7.rs:229-262): device-resident snapshot of one batch, f32 [D, S+2, L] in `buf`
 * (stream-ordered device-to-device copies, no host round trip: multi-session serving keeps snapshots in HBM) */
int32_t wrk_v7_state_read(wrk_ctx* ctx, const wrk_v7_state* state, uint32_t batch, wrk_buf* buf);
int32_t wrk_v7_state_write(wrk_ctx* ctx, wrk_v7_state* state, uint32_t batch, const wrk_buf* buf);

/* One RnnJob (load + submit + back, v7.rs:434-492) for a chunk of `num_token` stacked tokens.
 *   tokens     u32 [num_token] ids (device gather from emb_f16), or NULL with
 *   emb_rows   f16 [D, num_token] rows gathered by the caller (Token::Embed / CPU gather)
 *   cursors    packed Cursor per token (tensor/mod.rs:53-60)
 *   headers    stacked row indices fed to the head (RnnRedirect::headers, rnn.rs:41-81)
 *   logits     host f32 [num_vocab, num_header] or NULL
 *   argmax     host u32 [num_header] or NULL (greedy token per header row, computed on device)
 *   mode       0 = op-by-op (one kernel per reference TensorOp, the launch list of v7.rs:716-1007);
 *              1 = fast paths: one token per sequence -> the fused 5-launch decode layer; multi-token chunks -> the
 *                  same op list with merged launches (six shifts in one pass, projections grouped per stage, the
 *                  element-wise chains around the WKV kernel as one kernel each, residual adds in the GEMM epilogue),
 *                  whose logits and state are bit-identical to mode 0 above 64 stacked tokens
 */
int32_t wrk_v7_infer(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state,
                     const uint32_t* tokens, const uint16_t* emb_rows, const uint32_t* cursors, uint32_t num_token,
                     const uint32_t* headers, uint32_t num_header, float* logits, uint32_t* argmax, uint32_t mode);

/* Bundle::<F>::new (v7.rs:514-536; Runtime<F> v7.rs:281-364 is generic over the activation type): WRK_F16 = Bundle::<f16>, the
 * reference's default build; WRK_F32 = Bundle::<f32>: every frame buffer but `input` holds f32, matmuls read f32 inputs
 * (IN_FP32 shader variants), the op-by-op launch list runs whatever `mode` says.  Call between jobs; drops cached programs. */
int32_t wrk_v7_model_set_frame_dtype(wrk_ctx* ctx, wrk_v7_model* model, uint32_t dtype);

/* The persistent batch-1 decode engine (one launch for all layers of a token; the device-side analogue of the reference's
 * speculative job queue, runtime/mod.rs:110-209, which keeps the next job ready while the current one runs).  It is built on the
 * first one-token job of a model and used by mode 1 whenever it exists and WRK_ENGINE != 0.  Returns 1 when the engine exists,
 * 0 when it does not (reason copied to `why`, NUL-terminated, when why != NULL), < 0 on error.  Builds it if no job has run yet. */
int32_t wrk_v7_model_engine_status(wrk_ctx* ctx, wrk_v7_model* model, char* why, size_t capacity);

/* Parity instrumentation at the reference's own seam: v7::Hook / HookMap closures receive the `Frame` (state + Runtime<F>
 * buffers) at every stage of a layer (v7.rs:386-421, 497-502) and examples/inspect.rs:100-248 reads each buffer back per layer.
 *   wrk_v7_infer_layer: run ONLY `layer` of a job (mode as wrk_v7_infer) on a caller-supplied layer input x [D, num_token] and
 *                       layer-0 value v_first [D, num_token] (NULL for layer 0), both in the frame dtype; the state slice of the layer advances
 *   wrk_v7_frame_read : TensorGpu::back of one frame buffer, by inspect.rs's name (x, att_x, att_r, att_w, att_k, att_v, att_a, att_g,
 *                       att_o, att_kk, att_vv, att_n, att_rx ... att_gx, aux_w/a/g/v, ffn_x, ffn_kx, ffn_k, ffn_v; att_x_ln = LN1(x) of the
 *                       fused decode path); dst NULL returns the size.  In mode 1 only the buffers the fused kernels materialise are meaningful. */
int32_t wrk_v7_infer_layer(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, uint32_t layer, const void* x, const void* v_first,
                           const uint32_t* cursors, uint32_t num_token, uint32_t mode);
int32_t wrk_v7_frame_read(wrk_ctx* ctx, wrk_v7_model* model, const char* name, uint32_t num_token, void* dst, size_t capacity, size_t* bytes);

/* Greedy decode loop kept on the device (the reference's bench loop, examples/bench.rs:224-236,
 * with softmax+argmax moved on device): every sequence b feeds `first_tokens[b]`, then its own
 * argmax, for `steps` steps.  out_tokens: host u32 [steps, num_batch] or NULL.  One hipGraph per
 * step shape is built on first use and replayed.  elapsed_ms_or_null receives the HIP-event time
 * of the `steps` replays on the context's stream.
 * mode: bits 0-7 as wrk_v7_infer (0 op-by-op, 1 fused); bits 8-15 = G > 1: the num_batch INDEPENDENT sequences (separate state
 * slices, v7.rs:519-521) are dealt in contiguous blocks over G concurrent pipelines -- each with its own Runtime<F> frame, cached
 * step program and HIP stream, all sharing the one set of weights -- so that several latency-bound decode pipelines overlap on the
 * GPU (the in-GPU analogue of sharding streams over GPUs; results equal running each block on its own). */
int32_t wrk_v7_generate_greedy(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state,
                               const uint32_t* first_tokens, uint32_t num_batch, uint32_t steps,
                               uint32_t* out_tokens, float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);

/* examples/chat.rs:150-190 Sampler::sample on the device, one token per row of f32 logits [num_rows][row_stride] (first num_vocab used):
 * softmax, nucleus = the tokens (by probability descending, ties by index ascending) whose preceding mass is <= top_p, weights p^(1/T)
 * inside it, then the first token whose cumulative weight reaches u * total, u = SplitMix64((seed << 32) | step) >> 40, times 2^-24.
 * temperature or top_p == 0: the first index of the maximum (greedy); NaN or negative, or a temperature of +inf: WRK_E_ARG (every
 * entry point that takes a temperature, the decode loops included; top_p may be +inf: no cut); num_vocab > 2^20: WRK_E_UNSUPPORTED.
 * A logit of NaN counts as -inf, -0 as +0; with a +inf in the row the draw is among the +inf tokens alone, each with weight 1.
 * temperature / top_p / seed: host arrays of num_rows.  Blocking; out_tokens: host u32 [num_rows]. */
int32_t wrk_sample_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                          const float* temperature, const float* top_p, const uint32_t* seed, uint32_t step, uint32_t* out_tokens);
/* as wrk_v7_generate_greedy, the next token of sequence b drawn as wrk_sample_logits does with (temperature[b], top_p[b], seed[b]) at
 * step t = 0..steps-1 of this call.  The parameters are uploaded per call: one cached step program serves any parameters. */
int32_t wrk_v7_generate_sample(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                               uint32_t steps, const float* temperature, const float* top_p, const uint32_t* seed,
                               uint32_t* out_tokens, float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);
/* wrk_sample_logits with two more cuts of the candidates per row (ChatRWKV / ai00 top_k, llama.cpp min_p).  In wrk_sample_logits' order
 * the candidates are the first min(n_P, n_K, n_M) ranks: n_P the nucleus count (against the whole row's softmax mass: not renormalised
 * after the other cuts; top_p >= 1: num_vocab); n_K = top_k (0 or >= num_vocab: off; exactly top_k tokens survive, ties broken by index);
 * n_M = the number of tokens with fl32(l - max) >= fl32(ln(min_p)) (the subtraction in f32, the logarithm taken in f64 on the host and
 * rounded once; min_p == 0: off; rank 0 always passes).  Weights p^(1/T) inside the candidates, the draw as wrk_sample_logits'.
 * top_k == 1 is the greedy branch.  top_k: host u32 [num_rows], min_p: host f32 [num_rows] in [0, 1] (NaN or outside: WRK_E_ARG); either
 * may be NULL (off).  With both off every token equals wrk_sample_logits', bit for bit. */
int32_t wrk_sample_logits_filtered(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                                   const float* temperature, const float* top_p, const uint32_t* top_k, const float* min_p,
                                   const uint32_t* seed, uint32_t step, uint32_t* out_tokens);
/* Mirostat v2 (Basu et al. 2021, Alg. 2; llama.cpp mirostat_v2) per row, on wrk_sample_logits' row l (NaN as -inf, -0 as +0), its maximum
 * mx, its order and its u.  Row parameters: tau > 0 (target surprise, bits), eta >= 0 (learning rate) and the state mu (f32).  With
 *   w_i = exp((l_i - mx) / T), W = sum_i w_i, s_i = log2 W - (l_i - mx) / T * log2 e
 * the candidates are rank 0 and every token with s_i <= mu (a prefix of the order); the drawn token y is the first rank whose cumulative
 * weight reaches u * W_c, W_c = the candidates' weight; its observed surprise s = log2 W_c - (l_y - mx) / T * log2 e is renormalised over
 * the candidates (one candidate: s == 0 exactly); then mu <- mu - eta * (s - tau).  top_p is not read by such a row.  tau[r] == 0 turns
 * Mirostat off for the row: wrk_sample_logits' token, top_p included, bit for bit, and mu untouched.  temperature == 0 and an all -inf
 * row are the greedy branch, which leaves mu untouched as well.  tau / eta: host f32 [num_rows] (eta NULL: 0); mu_inout: host f32
 * [num_rows], the mu each row starts from and, on return, the mu after its draw; NULL: every row starts at 2 tau, a fresh sequence, and
 * nothing is returned.  WRK_E_ARG before any launch: NaN, negative or non-finite tau / eta, a non-finite mu, a NULL tau.  Blocking. */
int32_t wrk_sample_logits_mirostat(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                                   const float* temperature, const float* top_p, const float* tau, const float* eta, float* mu_inout,
                                   const uint32_t* seed, uint32_t step, uint32_t* out_tokens);
/* Locally typical sampling (Meister et al. 2022; HF TypicalLogitsWarper, llama.cpp typical_p) per row, on the same row, order and u.
 * With p = softmax(l) at temperature 1, g_i = mx - l_i and gbar = sum_i p_i g_i, a token's distance to the entropy is
 * d_i = |-ln p_i - H| = |g_i - gbar| (a -inf logit adds 0 to gbar and has d = +inf).  In the typical order -- d ascending, ties by index
 * ascending -- the token at rank r is a candidate iff the mass sum p before it is <= typical_p: the token that crosses is in, rank 0
 * always.  The draw is among the candidates in wrk_sample_logits' order with weights p^(1/T).  top_p is not read by such a row.
 * typical_p[r] >= 1 turns the cut off for the row: wrk_sample_logits' token, top_p included, bit for bit.  temperature == 0 and an
 * all -inf row are the greedy branch.  typical_p: host f32 [num_rows] in [0, 1] (NaN or outside, or NULL: WRK_E_ARG).  Blocking. */
int32_t wrk_sample_logits_typical(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                                  const float* temperature, const float* top_p, const float* typical_p, const uint32_t* seed,
                                  uint32_t step, uint32_t* out_tokens);
/* wrk_sample_logits_filtered with four more cuts per row: top-n-sigma (Tang et al. 2024; llama.cpp top_n_sigma), the epsilon and eta
 * cut-offs (Hewitt et al. 2022; Hugging Face EpsilonLogitsWarper / EtaLogitsWarper) and XTC, "exclude top choices" (koboldcpp,
 * text-generation-webui, llama.cpp).  p is the whole row's softmax at temperature 1, never renormalised after another cut (llama.cpp
 * renormalises over the survivors before XTC).  In wrk_sample_logits' order the candidates are the ranks [m0, n).
 *   n = min(n_P, n_K, n_M, n_S, n_E, n_H), each of the last three a prefix with rank 0 always in:
 *     n_S = #{l >= max - top_n_sigma * sigma}, sigma the population standard deviation of the row's finite logits (fewer than two, or
 *           a +inf in the row: 0 -- the ties of the maximum stay); top_n_sigma <= 0: off, +inf counts as the largest finite f32;
 *     n_E = #{p >= epsilon_cutoff}; 0: off;
 *     n_H = #{p >= min(eta_cutoff, sqrt(eta_cutoff) * exp(-H))}, H the row's entropy in nats (a -inf logit adds 0); 0: off.
 *   XTC: m = #{p >= xtc_threshold}, m' = min(m, n); the row's coin c is the second output of the SplitMix64 stream whose first gives u,
 *     c = (SplitMix64 state (seed << 32 | step) advanced twice) >> 40, times 2^-24.  m' >= 2 and c < xtc_probability: m0 = m' - 1 -- every
 *     candidate at or above the threshold goes except the least likely of them; else m0 = 0.  xtc_probability == 0 or xtc_threshold >
 *     0.5: off.  [m0, n) is never empty.
 * Weights p^(1/T) inside the candidates, the draw as wrk_sample_logits'.  temperature == 0, top_p == 0, top_k == 1 and an all -inf row
 * are the greedy branch: no cut applies, no coin is drawn.  The thresholds are compared as f32 bounds on l - max, their logarithms
 * taken in f64 on the host and rounded once.  Every array is host f32 [num_rows] and may be NULL (off), xtc_probability and
 * xtc_threshold both or neither; WRK_E_ARG before any launch: a NaN or negative value, an epsilon_cutoff, eta_cutoff, xtc_probability
 * or xtc_threshold outside [0, 1].  With all five off every token equals wrk_sample_logits_filtered's, bit for bit.  Blocking. */
int32_t wrk_sample_logits_cut(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                              const float* temperature, const float* top_p, const uint32_t* top_k, const float* min_p,
                              const float* top_n_sigma, const float* epsilon_cutoff, const float* eta_cutoff, const float* xtc_probability,
                              const float* xtc_threshold, const uint32_t* seed, uint32_t step, uint32_t* out_tokens);

/* Sequence scoring on the device, per row of f32 logits [num_rows][row_stride] (first num_vocab used) and its target token t:
 *   logprob = x_t - (m + log sum_i exp(x_i - m)), m = the row max;   rank = #{i : x_i > x_t} + #{i < t : x_i == x_t}
 * so rank == 0 exactly when t is the greedy token (the first index of the maximum).  A NaN anywhere in the row gives logprob NaN
 * (rank unspecified); a target logit of -inf gives -inf.  targets: host u32 [num_rows], each < num_vocab (else WRK_E_ARG).
 * Blocking; logprob: host f32 [num_rows], rank: host u32 [num_rows].  Same bits for the same (num_rows, num_vocab, row_stride). */
int32_t wrk_score_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                         const uint32_t* targets, float* logprob, uint32_t* rank);
/* Log-probs of chosen tokens and their most likely alternatives, per row x of f32 logits [num_rows][row_stride] (first num_vocab used)
 * and its chosen token y = tokens[row] (OpenAI's logprobs / top_logprobs, vLLM's logprobs=N):
 *   logprob         = (x_y - m) - log sum_i exp(x_i - m), m = the row max: wrk_score_logits' expression
 *   top_ids[j]      = the j-th token in wrk_sample_logits' order: logit descending, ties by index ascending (j < num_top)
 *   top_logprobs[j] = the same expression at top_ids[j]
 * The row is the raw head output at temperature 1, before penalties, bans and filters -- what last_logits returns and wrk_score_logits
 * scores: a banned or filtered-out token may appear among the alternatives, and the chosen token of a sampled or penalised pick gets
 * its probability under the model, not under the sampler.  A logit of -inf has log-prob -inf and sorts after every finite logit, by
 * index.  With num_top > num_vocab the entries j >= num_vocab are id 0xFFFFFFFF and log-prob -inf.  A NaN anywhere in the row gives NaN
 * in logprob and in every top_logprobs entry; the ids of such a row are unspecified.  When y is the first index of the maximum (a greedy
 * pick) top_ids[0] == y and top_logprobs[0] has the bits of logprob.  Same bits for the same (num_rows, num_vocab, row_stride, num_top).
 * 0 <= num_top <= WRK_MAX_TOP_LOGPROBS; with 0 only logprob is produced and the top arrays may be NULL.  tokens: host u32 [num_rows].
 * Blocking; logprob: host f32 [num_rows], top_ids: host u32 [num_rows][num_top], top_logprobs: host f32 [num_rows][num_top].
 * WRK_E_ARG before any launch: a token >= num_vocab, num_top > WRK_MAX_TOP_LOGPROBS, a NULL required array.  num_vocab > 2^20:
 * WRK_E_UNSUPPORTED (the sampler's limit). */
#define WRK_MAX_TOP_LOGPROBS 20
int32_t wrk_top_logprobs(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                         const uint32_t* tokens, uint32_t num_top, float* logprob, uint32_t* top_ids, float* top_logprobs);
/* as wrk_v7_infer, with the header rows scored instead of read back: header row h gets wrk_score_logits' (logprob[h], rank[h]) of
 * target targets[h] (host u32 [num_header], each < num_vocab, required when num_header > 0).  The state advances exactly as
 * wrk_v7_infer's on the same job; only num_header floats and u32 come back.  Targets are device data: one cached program per job shape
 * serves any targets (score jobs never share a program with infer jobs).  Not inside a capture. */
int32_t wrk_v7_score(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state,
                     const uint32_t* tokens, const uint16_t* emb_rows, const uint32_t* cursors, uint32_t num_token,
                     const uint32_t* headers, uint32_t num_header, const uint32_t* targets, float* logprob, uint32_t* rank, uint32_t mode);

/* Repetition penalties (ChatRWKV PIPELINE.generate: alpha_presence / alpha_frequency / alpha_decay / token_ban) on the device.
 * An occurrence table has num_batch slots of num_vocab entries (slot b belongs to state slot b): count[n] f32 and flags[n] (bit 0
 * present, bit 1 banned), plus one weight vector w[n] (finite, >= 0, default 1: ChatRWKV's `www`).  A row x of slot b is penalised as
 *   x'[n] = -inf if banned[n];  x[n] - (presence + count[n] * frequency) if present[n] (t = count * frequency; t = presence + t;
 *   x - t, each rounded to f32);  x[n] otherwise
 * and a drawn token y updates the slot as: count[n] *= decay for every n; then count[y] += w[y]; then present[y] = 1.
 * Flags cross the ABI as one uint32_t per token.  Every call validates on the host first (WRK_E_ARG): NULL arrays, slots out of range,
 * tokens >= num_vocab, a table of another context, non-finite presence / frequency, decay outside [0, 1], weights < 0 or non-finite,
 * and any ban or load that would leave a slot with no allowed token.  num_vocab > 2^20: WRK_E_UNSUPPORTED (the sampler's limit). */
typedef struct wrk_occurrence wrk_occurrence;
int32_t wrk_occurrence_create(wrk_ctx* ctx, uint32_t num_batch, uint32_t num_vocab, wrk_occurrence** out);   /* zero counts and flags */
int32_t wrk_occurrence_destroy(wrk_occurrence* occ);
/* weights: host f32 [num_vocab], or NULL for all 1 */
int32_t wrk_occurrence_set_weights(wrk_ctx* ctx, wrk_occurrence* occ, const float* weights);
/* sets (banned != 0) or clears the banned bit of tokens[0..n) in slot `batch` */
int32_t wrk_occurrence_ban(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t batch, const uint32_t* tokens, uint32_t n, int32_t banned);
/* applies the update rule for tokens[0], tokens[1], ... in order (e.g. to count a prompt) */
int32_t wrk_occurrence_add(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t batch, const uint32_t* tokens, uint32_t n, float decay);
/* counts: host f32 [num_vocab], flags: host u32 [num_vocab] */
int32_t wrk_occurrence_back(wrk_ctx* ctx, const wrk_occurrence* occ, uint32_t batch, float* counts, uint32_t* flags);
/* counts (finite) and flags (values 0..3) of one slot; both NULL: reset the slot to zero counts and no flags */
int32_t wrk_occurrence_load(wrk_ctx* ctx, wrk_occurrence* occ, uint32_t batch, const float* counts, const uint32_t* flags);
/* penalises f32 logits [num_rows][row_stride] (first num_vocab used) in place; row r uses slot first_batch + r and presence[r] /
 * frequency[r] (host f32 [num_rows]).  Blocking.  In a host-side chat loop it goes between infer and wrk_sample_logits. */
int32_t wrk_penalize_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                            const wrk_occurrence* occ, uint32_t first_batch, const float* presence, const float* frequency);
/* as wrk_v7_generate_sample, the draw of sequence b made on its logits penalised with slot b of `occ` and (presence[b], frequency[b]),
 * and slot b updated with decay[b] after every draw (host f32 [num_batch]).  The first token of a call is not counted; the last drawn
 * token is.  last_logits stays the head output before penalties.  The table is passed to the step program as data: one cached program
 * serves any table and any parameters; occ->num_batch >= num_batch and occ->num_vocab == the model's. */
int32_t wrk_v7_generate_penalized(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                                  uint32_t steps, const float* temperature, const float* top_p, const uint32_t* seed, const float* presence,
                                  const float* frequency, const float* decay, wrk_occurrence* occ, uint32_t* out_tokens,
                                  float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);

/* Constrained decoding ("structured output": ai00's BNF sampler, vLLM's guided_choice / guided_regex, llama.cpp's grammars, below their
 * compilers): a deterministic automaton over token ids, supplied by the caller, says which tokens a row may draw as a function of what
 * it drew before.  Alphabet compression: token_class[num_vocab] (u16) maps every token to one of num_classes classes, and
 * transitions[num_states][num_classes] (u16) holds the next state, or WRK_GRAMMAR_REJECT when the class is not allowed in that state;
 * with num_classes == num_vocab and the identity map this is the dense table.  1 <= num_states <= 65535, 1 <= num_classes <=
 * WRK_MAX_TOKEN_CLASSES (one state's row is at most 16 KB: it is staged in LDS), num_vocab <= 2^20 (the sampler's limit, beyond it
 * WRK_E_UNSUPPORTED).  WRK_E_ARG before anything is uploaded: NULL arrays, a class >= num_classes, a next state that is neither
 * < num_states nor WRK_GRAMMAR_REJECT, and a state in which no token is allowed (no class that at least one token maps to has a next
 * state) -- so a row masked by a grammar alone is never empty.  A grammar that is "finished" says so itself: its final state allows
 * only the caller's end token and loops on it.  Both arrays are copied: the caller's may go after the call. */
#define WRK_GRAMMAR_REJECT 0xFFFFu
#define WRK_MAX_TOKEN_CLASSES 8192
typedef struct wrk_grammar wrk_grammar;
int32_t wrk_grammar_create(wrk_ctx* ctx, uint32_t num_vocab, uint32_t num_states, uint32_t num_classes, const uint16_t* token_class,
                           const uint16_t* transitions, wrk_grammar** out);
int32_t wrk_grammar_destroy(wrk_grammar* grammar);
/* masks f32 logits [num_rows][row_stride] (first num_vocab used) in place: row r keeps logits[r][v], bits unchanged (NaN payloads
 * included), if token v is allowed in states[r], and gets -inf otherwise.  states: host u32 [num_rows], each < num_states (else
 * WRK_E_ARG).  Blocking.  In a host-side loop it goes between wrk_penalize_logits and wrk_sample_logits. */
int32_t wrk_constrain_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                             const wrk_grammar* grammar, const uint32_t* states);
/* states[r] <- transitions[states[r]][token_class[tokens[r]]] on the device; a rejected token leaves states[r] as it was.  states: host
 * u32 [num_rows], in/out; tokens: host u32 [num_rows], each < num_vocab.  Blocking. */
int32_t wrk_grammar_advance(wrk_ctx* ctx, const wrk_grammar* grammar, uint32_t* states, const uint32_t* tokens, uint32_t num_rows);

/* Regex -> token automaton (vLLM's guided_regex).  Two steps: patterns -> a byte DFA on the host, byte DFA x vocabulary
 * -> a wrk_grammar on the device.  The tokenizer stays outside: the vocabulary is one byte string per token id.
 *
 * wrk_regex_compile needs no context and no device.  The alphabet is bytes, matching is whole-string.  Dialect: literals (a code point
 * outside ASCII is its UTF-8 bytes), \ before a metacharacter, \n \r \t \f \v, \xHH (one raw byte), \d \w \s (ASCII; \s is
 * [ \t\n\r\f\v]) and \D \W \S (any other code point, every well-formed multi-byte UTF-8 sequence included), "." (a code point other
 * than \n), [...] and [^...] over ASCII members, ASCII ranges and the class escapes (a negated class matches every other code point),
 * groups (...) and (?:...), | (empty alternatives allowed), * + ? {m} {m,} {m,n} with n <= 1000.  WRK_E_UNSUPPORTED, with the
 * construct and its byte offset in err ("pattern 0: unsupported: look-around at offset 3"): anchors and \b \B \A \Z, back-references,
 * look-around, lazy or possessive quantifiers, named groups, inline flags, \p{..}, a class member outside ASCII, a repeat count above
 * 1000, more than 65 534 states in total.  WRK_E_ARG with "syntax: ... at offset N": everything else that does not parse.  err may be
 * NULL.  Pattern p's DFA is minimal and trimmed (every state reachable from its start, an accepting state reachable from every state;
 * no dead state: a missing transition is WRK_GRAMMAR_REJECT), numbered breadth-first from its start in byte order; the state sets are
 * disjoint and concatenated in pattern order, starts[p] the first state of pattern p.
 * wrk_byte_dfa_from_arrays makes the same object from next[num_states][256] (a state or WRK_GRAMMAR_REJECT), accepting[num_states] and
 * starts[num_patterns]: the entry for a BNF or JSON-schema compiler of the caller's.  Ranges are checked (WRK_E_ARG), nothing else;
 * 1 <= num_states <= 65 534.  wrk_byte_dfa_export: the counts, and the arrays into whichever pointers are not NULL. */
typedef struct wrk_byte_dfa wrk_byte_dfa;
int32_t wrk_regex_compile(const char* const* patterns, const size_t* lengths, uint32_t num_patterns, wrk_byte_dfa** out, char* err,
                          size_t err_cap);
int32_t wrk_byte_dfa_from_arrays(uint32_t num_states, const uint16_t* next, const uint8_t* accepting, const uint32_t* starts,
                                 uint32_t num_patterns, wrk_byte_dfa** out);
int32_t wrk_byte_dfa_export(const wrk_byte_dfa* dfa, uint32_t* num_states, uint32_t* num_patterns, uint16_t* next_or_null,
                            uint8_t* accepting_or_null, uint32_t* starts_or_null);
void wrk_byte_dfa_destroy(wrk_byte_dfa* dfa);
/* The token automaton of a byte DFA over a vocabulary: token t is the bytes [vocab_offsets[t], vocab_offsets[t + 1]) of vocab_bytes.
 * Its states are the byte-DFA states plus one FINAL state, the last.  From state s token t leads where its bytes lead; a missing byte
 * transition on the way is REJECT, and an empty token is REJECT everywhere.  end_token's bytes are ignored: it leads from an accepting
 * state to FINAL, is REJECT elsewhere, and FINAL allows only end_token and loops on it.  Then every state from which FINAL cannot be
 * reached through tokens of this vocabulary is dropped and the transitions into it become REJECT, so every state allows a token; kept
 * states keep their order, renumbered compactly; columns that are then equal share a class, classes numbered by first token id.
 * start_states[p] (num_patterns of the DFA) and *final_state are the new numbers.  The walk runs on the device (wrk_grammar_compile.hip)
 * in scratch of O(vocabulary bytes + num_vocab + states x byte classes + states x classes); the result is exact.  Blocking.
 * WRK_E_ARG before any launch: NULL arguments, num_vocab 0, end_token >= num_vocab, offsets that decrease; after the walk: "the
 * vocabulary cannot spell pattern p".  WRK_E_UNSUPPORTED: num_vocab > 2^20; more than WRK_MAX_TOKEN_CLASSES distinct token columns
 * over the byte-DFA states (counted before the trim, which bounds the scratch).  The grammar is an ordinary wrk_grammar.
 * wrk_grammar_compile_last_ms: the wall-clock milliseconds of this thread's last wrk_grammar_compile, per phase: byte classes and
 * mapping, upload + hash pass, representative walks, verify passes, trim, create.
 * wrk_grammar_export reads a grammar's tables back: the counts, and the arrays into whichever pointers are not NULL.  Blocking. */
#define WRK_GRAMMAR_COMPILE_PHASES 6
int32_t wrk_grammar_compile(wrk_ctx* ctx, const wrk_byte_dfa* dfa, uint32_t num_vocab, const uint8_t* vocab_bytes,
                            const uint64_t* vocab_offsets, uint32_t end_token, wrk_grammar** out, uint32_t* start_states,
                            uint32_t* final_state);
int32_t wrk_grammar_compile_last_ms(float* ms);
int32_t wrk_grammar_export(const wrk_grammar* grammar, uint32_t* num_states, uint32_t* num_classes, uint16_t* token_class_or_null,
                           uint16_t* transitions_or_null);

/* Logit bias (ai00's `bias`, llama.cpp's --logit-bias, the first link of its sampler chain, vLLM's and the OpenAI interfaces'
 * logit_bias, whose -100 is -inf here): a wrk_logit_bias is an immutable, device-resident collection of num_sets bias sets over one
 * vocabulary.  Set s is the pairs (ids[e], values[e]) for e in [set_offsets[s], set_offsets[s + 1]) (num_sets + 1 offsets); the three
 * arrays are copied, the caller's may go after the call.  1 <= num_sets <= WRK_MAX_BIAS_SETS, num_vocab <= 2^20 (the sampler's limit,
 * beyond it WRK_E_UNSUPPORTED).  A set may be empty and may have up to num_vocab entries: there is no per-set cap.  WRK_E_ARG before
 * anything is uploaded: NULL arrays, offsets that do not start at 0 or that decrease, an id >= num_vocab, the same id twice in one set,
 * a value that is NaN or +inf, and a set that bans every token of the vocabulary -- so a row biased by a set alone is never empty, as
 * for a grammar. */
#define WRK_BIAS_NONE 0xFFFFFFFFu
#define WRK_MAX_BIAS_SETS 65536
typedef struct wrk_logit_bias wrk_logit_bias;
int32_t wrk_logit_bias_create(wrk_ctx* ctx, uint32_t num_vocab, uint32_t num_sets, const uint32_t* set_offsets, const uint32_t* ids,
                              const float* values, wrk_logit_bias** out);
int32_t wrk_logit_bias_destroy(wrk_logit_bias* bias);
/* biases f32 logits [num_rows][row_stride] (first num_vocab used) in place: row r with set s = sets[r] gets -inf at every token of s
 * whose value is -inf, whatever the logit is (a ban is a ban, as the occurrence table's: not x + (-inf), which is NaN for x = +inf),
 * and x + v, one IEEE f32 addition, at every token of s with a finite value v (NaN stays NaN, +-inf stay +-inf); every other token
 * keeps its bits, NaN payloads and -0 included, and a row with sets[r] == WRK_BIAS_NONE is left as it is.  sets: host u32 [num_rows],
 * each < num_sets or WRK_BIAS_NONE (else WRK_E_ARG, as for an object of another context or another num_vocab).  Blocking.  In a
 * host-side loop it goes in front of wrk_penalize_logits. */
int32_t wrk_bias_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                        const wrk_logit_bias* bias, const uint32_t* sets);

/* Classifier-free guidance (Hugging Face's guidance_scale with negative_prompt_ids, llama.cpp's --cfg-scale with --cfg-negative-prompt,
 * text-generation-webui's negative prompt): the row a pick is made on is mixed from the row of the sequence itself (conditional, xc) and
 * the row of a partner sequence that was fed the negative prompt (unconditional, xu).  The rows are mixed raw, without a log-softmax:
 * that differs from lu + s * (lc - lu) on log-softmaxed rows by one constant per row, which the arg-max, every sampler family, bias,
 * penalties, DRY and the grammar mask do not see.  With c = xc and u = xu after NaN -> -inf and -0 -> +0, and the row's scale s, the
 * first case that applies: s == 1: the bits of xc, unchanged (the row is off; NaN payloads and -0 included); c == -inf: -inf (impossible
 * under the prompt stays impossible); c == +inf: +inf; u == -inf: c; s == 0: u; u == +inf: -inf if s > 1, else +inf; otherwise
 * d = c - u, p = s * d, out = p + u, three separate IEEE f32 operations, never a fused multiply-add; when d or p overflows the result
 * is that infinity.  Outside s == 1 rows the result is never NaN.
 * wrk_guide_logits: logits holds 2 * num_rows f32 rows of row_stride (first num_vocab used), the num_rows conditional ones first, row
 * num_rows + r the partner of row r; out receives num_rows rows of out_stride, another buffer; nothing between the rows of out is
 * written.  scale: host f32 [num_rows], each finite and >= 0 (else WRK_E_ARG, from every call that takes one); num_vocab > 2^20:
 * WRK_E_UNSUPPORTED.  Blocking.  In a host-side loop it goes in front of wrk_bias_logits. */
int32_t wrk_guide_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                         const float* scale, wrk_buf* out, uint32_t out_stride);

/* DRY ("don't repeat yourself": text-generation-webui, koboldcpp, llama.cpp's dry_multiplier / dry_base / dry_allowed_length /
 * dry_sequence_breakers) and the hard ban of the same match (Hugging Face's no_repeat_ngram_size), on the device.  Both look at the ORDER
 * of what a sequence generated, which the occurrence table cannot: a token window has num_batch slots (slot b belongs to state slot b),
 * each the last `capacity` tokens that counted, oldest first, kept as a ring on the device; a push into a full slot drops the oldest.
 * 1 <= capacity <= WRK_MAX_TOKEN_WINDOW, every stored id < num_vocab, num_vocab <= 2^20 (beyond it WRK_E_UNSUPPORTED).
 * Match length.  A row has the window w[0..n), last = w[n-1], and the call-wide breaker set Bk (at most WRK_MAX_DRY_BREAKERS ids).
 * If n < 2 or last is in Bk nothing matches.  Else for every i in [0, n-2] with w[i] == last and t = w[i+1] not in Bk: m = 1; while
 * m < WRK_DRY_MAX_MATCH and i - m >= 0 and w[i-m] == w[n-1-m] and w[n-1-m] is not in Bk, m += 1; M[t] = max(M[t], m).  Tokens never
 * reached have M = 0.  (text-generation-webui's loop with llama.cpp's cap.)
 * Row parameters: multiplier finite >= 0, base finite >= 1, allowed_length in [1, WRK_DRY_MAX_MATCH], no_repeat_ngram 0 or in
 * [2, WRK_DRY_MAX_MATCH + 1]; anything else is WRK_E_ARG.  The host computes pen[m] = 0 for m < allowed_length, else p_0 = (double)
 * multiplier, p_{k+1} = p_k * (double)base (one f64 rounding per product), pen[m] = min(FLT_MAX, (float)p_{m - allowed_length}): the
 * same table on every IEEE host, and a finite penalty never meets a +inf logit as inf - inf.
 * Row result for token t with M = M[t]: -inf if no_repeat_ngram != 0 and M >= no_repeat_ngram - 1; else x[t] - pen[M] (one f32
 * subtraction) if multiplier != 0 and M >= allowed_length; else the input bits unchanged (NaN payloads and -0 included).  With no
 * breakers the ban is exactly no_repeat_ngram_size over the window; a row with multiplier == 0 and no_repeat_ngram == 0 is its input
 * bit for bit. */
#define WRK_MAX_TOKEN_WINDOW 4096
#define WRK_MAX_DRY_BREAKERS 16
#define WRK_DRY_MAX_MATCH 50
typedef struct wrk_token_window wrk_token_window;
int32_t wrk_token_window_create(wrk_ctx* ctx, uint32_t num_batch, uint32_t num_vocab, uint32_t capacity, wrk_token_window** out);  /* empty slots */
int32_t wrk_token_window_destroy(wrk_token_window* window);
/* pushes tokens[0], tokens[1], ... into slot `batch` in order (e.g. a prompt); every id < num_vocab */
int32_t wrk_token_window_add(wrk_ctx* ctx, wrk_token_window* window, uint32_t batch, const uint32_t* tokens, uint32_t n);
/* tokens_out: host u32 [capacity], receives the slot's tokens oldest first; *len: how many */
int32_t wrk_token_window_back(wrk_ctx* ctx, const wrk_token_window* window, uint32_t batch, uint32_t* tokens_out, uint32_t* len);
/* the slot becomes tokens[0..n) (n <= capacity, oldest first); tokens NULL: the slot becomes empty */
int32_t wrk_token_window_load(wrk_ctx* ctx, wrk_token_window* window, uint32_t batch, const uint32_t* tokens_or_null, uint32_t n);
/* applies the row result above to f32 logits [num_rows][row_stride] (first num_vocab used) in place; row r uses slot first_batch + r
 * and multiplier[r], base[r], allowed_length[r], no_repeat_ngram[r] (host arrays [num_rows]; any may be NULL: 0 (off) / 1.75 / 2 / 0
 * (off)); breakers: host u32 [num_breakers], each < num_vocab, may be NULL with num_breakers 0.  The window is only read.  Blocking.
 * In a host-side loop it goes between wrk_penalize_logits and wrk_constrain_logits. */
int32_t wrk_dry_logits(wrk_ctx* ctx, wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_rows,
                       const wrk_token_window* window, uint32_t first_batch, const float* multiplier, const float* base,
                       const uint32_t* allowed_length, const uint32_t* no_repeat_ngram, const uint32_t* breakers, uint32_t num_breakers);

/* Stop tokens in the decode loops.  Sequence b has the stop set stop_tokens[stop_offsets[b] .. stop_offsets[b + 1]) (CSR, num_batch + 1
 * offsets, at most WRK_MAX_STOP_TOKENS ids each, every id < num_vocab).  Step i feeds x_i (x_0 = first_tokens[b]) and draws y_i; a
 * sequence that has not ended and whose y_i is in its stop set ends at step i: out_lengths[b] = i + 1 (the stop token is part of the
 * output); a sequence that never ends has out_lengths[b] = *steps_run.  out_tokens[j][b] for j < out_lengths[b] are the tokens the same
 * call without stop sets produces; rows out_lengths[b] .. *steps_run repeat the stop token; rows at or after *steps_run are not written.
 * After the call, state slot b is the state after consuming x_0 .. x_{out_lengths[b] - 1} (the stop token is drawn, not consumed): bit
 * for bit what a call without stops and steps = out_lengths[b] leaves.  With penalties, slot b of the table has counted exactly the
 * first out_lengths[b] tokens of the sequence.  last_logits[b] is the head output the last of those tokens was drawn from.
 * The host submits steps in blocks of poll_steps (0: the default) and stops once every sequence has ended: *steps_run <= steps, and
 * *steps_run <= (ceil(max(out_lengths) / poll_steps) + 2) * poll_steps.  While a sequence is still running, all `steps` run.
 * The pick is wrk_v7_generate_greedy's (temperature, top_p, seed all NULL), wrk_v7_generate_sample's, or with `occ`
 * wrk_v7_generate_penalized's (then the sampler arrays are required); both stop arrays NULL: no stops.  The stop sets are passed to
 * the step program as data: one cached program serves any stop sets.  WRK_E_ARG before any launch on: a NULL opt / out_lengths /
 * steps_run, offsets that do not start at 0 or decrease, more than WRK_MAX_STOP_TOKENS ids for a sequence, an id >= num_vocab, sampler
 * arrays only partly given, penalty arrays without a table, and whatever the three calls above reject.
 * top_k / min_p (host arrays [num_batch], either may be NULL: off) make the pick wrk_sample_logits_filtered's; they need the sampler
 * arrays (else WRK_E_ARG), and min_p outside [0, 1] is WRK_E_ARG.  With both stop arrays NULL this is the options form of
 * wrk_v7_generate_sample / wrk_v7_generate_penalized.  Filtered calls replay step programs of their own (any filter values: the rows
 * are device data); a call with both NULL runs exactly the programs it ran before.
 * Log-probs (wrk_top_logprobs on every step's head output, inside the step program): on iff out_logprob is non-NULL, host f32
 * [steps][num_batch]; with num_top > 0 (<= WRK_MAX_TOP_LOGPROBS, else WRK_E_ARG) out_top_ids (host u32) and out_top_logprobs (host f32)
 * [steps][num_batch][num_top] are required (else WRK_E_ARG).  Row j of sequence b belongs to y_j, scored on the raw head output it was
 * picked from.  Rows j < out_lengths[b] are what the same call without stop sets produces, the row of the stop token's own step
 * included; rows at or after out_lengths[b] are unspecified; rows at or after *steps_run are not written.  Tokens, lengths and states are
 * those of the call without log-probs.  num_top is data of the step program: one cached program serves any num_top; log-prob calls
 * replay step programs of their own, a call without them exactly the programs it ran before.  A sequence's log-probs do not depend on
 * the number of lanes.  The log-prob fields sit between poll_steps and the filter fields, which stay the last two: callers that name
 * their fields or start from a zeroed struct keep working after a recompile.
 * Mirostat v2 and locally typical sampling.  mirostat_tau (host f32 [num_batch]) makes the pick wrk_sample_logits_mirostat's with
 * (mirostat_tau[b], mirostat_eta[b]; eta NULL: 0) and a mu per sequence that lives in the step program from one draw to the next;
 * typical_p (host f32 [num_batch]) makes it wrk_sample_logits_typical's.  One call uses one family -- plain, filtered (top_k / min_p),
 * Mirostat or typical: arrays of two of them, mirostat_eta or mirostat_mu without mirostat_tau, or either new family without the sampler
 * arrays are WRK_E_ARG, as are the values the two row functions reject.  Both combine with penalties (the pick is made on the
 * penalised row), with stop sets and with log-probs (which stay on the raw head output).  mirostat_mu (host f32 [num_batch], in/out, may
 * be NULL): on entry the mu sequence b starts from (NULL: 2 tau, a fresh sequence), on return the mu after the draws of this call that
 * count -- the draws an occurrence row counts: every step up to and including the one that draws b's stop token, none after it, so
 * after the call mu[b] has seen exactly out_lengths[b] draws; a session carries mu from call to call through this array.  Tokens and
 * mu do not depend on the number of lanes.  The parameters are device data: one cached step program per family serves any values;
 * the two families replay step programs of their own, and a call with all four fields NULL runs exactly the programs it ran before.
 * The four fields sit between the log-prob fields and the filter fields, which stay the last two.
 * Constrained decoding.  `grammar` (NULL: off) masks the row every pick is made on as wrk_constrain_logits does with the sequence's
 * automaton state, and every draw that counts moves that state as wrk_grammar_advance does -- inside the step program.  Order within a
 * step: penalties, then the mask (in place on the penalised row, else into a copy of the head output), then the call's pick -- bit for
 * bit the pick of the same call on the masked row -- then log-probs, which stay on the raw head output (a disallowed token may appear
 * among the alternatives), then the tail.  With no sampler arrays the pick is the arg-max of the masked row: this entry point, with or
 * without stop sets, is constrained greedy.  The automaton sees exactly the draws an occurrence row counts and a Mirostat mu sees: every
 * step up to and including the one that draws b's stop token, none after it.  grammar_state (host u32 [num_batch], in/out, may be NULL):
 * on entry the state sequence b starts in (NULL: 0), on return the state after the draws that counted, out_lengths[b] of them; a session
 * carries it from call to call through this array.  WRK_E_ARG before any launch: grammar_state without grammar, a grammar of another
 * context or another num_vocab, a start state >= num_states.  The tables and the states are device data: one cached step program serves
 * any grammar and any start states; constrained calls replay step programs of their own, a call without a grammar exactly the programs
 * it ran before.  Tokens and final states do not depend on the number of lanes.  If the bans of `occ` and the automaton together leave
 * a row with no finite logit, the picked id is unspecified but < num_vocab (as for a NaN row); the automaton then sees a rejected token
 * and keeps its state, and nothing faults: to combine bans with a grammar, put them in the grammar.  The two fields sit between
 * the log-prob fields and the Mirostat fields: the six fields behind them, the filter fields last, stay where they were.
 * Stop sequences (multi-token stops: a stop string, tokenized by the caller, one sequence per way it tokenizes).  Next to its stop set,
 * sequence b has 0 .. WRK_MAX_STOP_SEQUENCES stop sequences of 1 .. WRK_MAX_STOP_SEQUENCE_LEN ids as a CSR of a CSR: stop sequence s is
 * stop_seq_tokens[stop_seq_offsets[s] .. stop_seq_offsets[s + 1]) and sequence b owns stop sequences [stop_seq_owners[b] ..
 * stop_seq_owners[b + 1]) (num_batch + 1 owners entries).  All three arrays or none; non-NULL arrays select the stop-sequence step
 * programs even when nobody owns a sequence, NULL arrays exactly the programs that ran before.  Every sequence has a tail: its last
 * WRK_STOP_TAIL_LEN draws that counted (the draws an occurrence row counts: every step up to and including the one that ends the
 * sequence, none after it; x_0 is not a draw), oldest first, right aligned, WRK_STOP_TAIL_EMPTY for a missing entry.  At a counted
 * draw y stop sequence k of length l matches when the last l entries of (tail ++ [y]) equal it; EMPTY equals no id, so nothing matches
 * across the start of the tail.  The sequence ends at that step if a stop sequence matches or y is in its stop set, exactly as a stop
 * token ends it: out_lengths, the frozen state slot, occurrence row, last_logits row, mu, grammar state and log-prob rows are those of
 * the call without stops run for out_lengths[b] steps.  out_stop_match (host u32 [num_batch], may be NULL): WRK_STOP_MATCH_NONE (not
 * ended by a stop), WRK_STOP_MATCH_TOKEN (an id of the stop set), else the index k of the matching stop sequence within b's list.  Of
 * several matches in one step the longest wins, at equal length the stop-set id beats a sequence and the lower index the higher.  The
 * host trims len(sequence k) tokens, or 1; the device trims nothing.  stop_tail (host u32 [num_batch][WRK_STOP_TAIL_LEN], in/out, may be
 * NULL: every tail starts empty and nothing is returned): a session carries its tail from call to call through this array, as it
 * carries mirostat_mu and grammar_state, so that a stop sequence that straddles two calls still ends the reply; the tail of a finished
 * sequence is frozen with it.  WRK_E_ARG before any launch: only some of the three arrays, offsets or owners that do not start at 0 or
 * decrease, more than WRK_MAX_STOP_SEQUENCES for one owner, a stop sequence of length 0 or above WRK_MAX_STOP_SEQUENCE_LEN, an id >=
 * num_vocab, out_stop_match or stop_tail without the three arrays, a stop_tail entry that is neither EMPTY nor < num_vocab, an EMPTY
 * entry after a non-EMPTY one.  The stop sequences are device data: one cached step program serves any of them.  Tokens, lengths,
 * matches and tails do not depend on the number of lanes.  The five fields sit between grammar_state and mirostat_tau.
 * DRY and the n-gram ban.  `window` (NULL: off) makes every pick see its row as wrk_dry_logits leaves it with slot b of the window and
 * (dry_multiplier[b], dry_base[b], dry_allowed_length[b], no_repeat_ngram[b]) (host arrays [num_batch], any may be NULL as there) and
 * the call-wide dry_breakers [num_dry_breakers], and every draw that counts is pushed into slot b -- inside the step program.  Order
 * within a step: penalties, then DRY (in place on the penalised row, else on a copy of the head output), then the grammar mask (in
 * place on that row), then the call's pick -- bit for bit the pick of the same call on that row; with no sampler arrays the arg-max,
 * the deterministic "no loops" mode -- then log-probs, which stay on the raw head output, then the tail.  The window takes a draw
 * exactly where an occurrence row counts it and a Mirostat mu moves: every step up to and including the one that ends the sequence,
 * none after it; x_0 is not pushed.  After the call slot b has taken exactly out_lengths[b] pushes; a session carries the window from
 * call to call in the handle.  A window with all four parameter arrays NULL still runs the DRY step programs and records the draws;
 * window NULL runs exactly the programs that ran before.  WRK_E_ARG before any launch: a parameter or breaker array without a
 * window, a window of another context or another num_vocab or with fewer slots than num_batch, more than WRK_MAX_DRY_BREAKERS
 * breakers, a breaker >= num_vocab, num_dry_breakers > 0 with dry_breakers NULL, the value ranges of wrk_dry_logits.  The window, the
 * tables and the breakers are device data: one cached step program serves any of them.  Tokens and final windows do not depend on the
 * number of lanes.  If bans, a grammar and the n-gram ban together leave a row with no finite logit, the picked id is unspecified but
 * < num_vocab and nothing faults.  The seven fields sit between out_top_logprobs and grammar.
 * Logit bias.  `bias` (NULL: off) makes every pick see its row as wrk_bias_logits leaves it with set bias_set[b] (host u32 [num_batch],
 * each < num_sets or WRK_BIAS_NONE; NULL: set 0 for every sequence) -- inside the step program.  Order within a step: bias first.  The
 * biased row is made from the raw head output in a buffer of its own, and everything that read the head output for the pick reads it
 * instead: penalties, then DRY, then the grammar mask, then the call's pick -- bit for bit the pick of the same call on that row; with
 * no sampler arrays the arg-max, so this entry point bans and prefers tokens in greedy decoding too.  A penalised, biased token is
 * (x + v) - t, in that order of rounding.  Log-probs, last_logits and the stop snapshot stay on the raw head output: a banned token may
 * appear among the alternatives.  The bias has no state: nothing moves from draw to draw and nothing is returned.  WRK_E_ARG before any
 * launch: bias_set without bias, an object of another context or another num_vocab, a set word that is neither < num_sets nor
 * WRK_BIAS_NONE.  The object and the set words are device data: one cached step program serves any object and any choice of sets;
 * biased calls replay step programs of their own, a call with bias NULL exactly the programs it ran before.  Tokens do not depend on
 * the number of lanes.  If a bias set, bans, a grammar and the n-gram ban together leave a row with no finite logit, the picked id is
 * unspecified but < num_vocab and nothing faults.  The two fields sit directly behind `occ`: every field behind them keeps its order.
 * Guidance.  guidance_scale (host f32 [num_batch]; NULL: off) makes sequence b a guided one: its partner is state slot num_batch + b,
 * into which the caller has fed the negative prompt, so the state needs 2 * num_batch slots (else WRK_E_ARG).  Every step runs both
 * slots, and the pick of b sees the row wrk_guide_logits makes of their two head rows with guidance_scale[b] -- inside the step program.
 * Order within a step: guidance first, in front of the bias; everything that read the head output for the pick reads the guided row
 * instead: bias, penalties, DRY, the grammar mask, then the call's pick -- bit for bit the pick of the same call on that row.  Log-probs,
 * last_logits and the stop snapshot stay on the raw head output of the conditional sequence.  The partner is fed b's draws: at step 0 it
 * feeds guidance_first_tokens[b] (host u32 [num_batch], each < num_vocab; NULL: first_tokens[b]), the last token of the negative prompt,
 * then y_0, y_1, ... as b does; it has b's stop set, stop sequences and tail, ends in the same step and is frozen as b is.  After the
 * call slot b is what the contract above says, and slot num_batch + b has consumed its own first token and the same draws: bit for bit
 * what a guided call without stops and steps = out_lengths[b] leaves in both.  out_tokens, out_lengths, last_logits, the log-prob rows,
 * mu, grammar states, matches and tails are num_batch wide, as without guidance; a call whose scales are all 1 returns, for sequences
 * [0, num_batch), bit for bit what the call without guidance on the same frame returns -- 2 * num_batch sequences, the partners' first
 * tokens behind the conditional ones; a call without guidance of num_batch sequences runs a smaller frame, whose matmul kernels round
 * differently: its logits agree to rounding, not bit for bit, and a near-tie may then pick another token.  WRK_E_ARG before any launch: guidance_first_tokens without guidance_scale, a scale that is NaN, infinite
 * or negative, a state of fewer than 2 * num_batch slots.  WRK_E_UNSUPPORTED before any launch: guidance on several lanes (mode bits
 * 8-15 > 1), in wrk_v7_generate_queue (wrk_queue_options' guidance_scale) and in wrk_v7_generate_beam (either field in `gen`).  The
 * scales are device data: one cached step program serves any of them; guided calls replay step programs of their own, a call with
 * guidance_scale NULL exactly the programs it ran before.  The two fields sit directly behind `bias_set` (the bias fields stay directly
 * behind `occ`, where callers and the binding checks know them): every field behind them keeps its order.
 * XTC, top-n-sigma and the eta / epsilon cut-offs.  top_n_sigma / epsilon_cutoff / eta_cutoff / xtc_probability / xtc_threshold (host f32
 * [num_batch], any may be NULL: off; the two XTC arrays both or neither) make the pick wrk_sample_logits_cut's with sequence b's values
 * and its top_k / min_p; the row's coin is a pure function of (seed[b], step), so nothing moves from draw to draw and nothing is
 * returned.  They need the sampler arrays and share the filtered family: together with mirostat_* or typical_p they are WRK_E_ARG, as
 * are the values wrk_sample_logits_cut rejects; num_vocab > 2^20 is WRK_E_UNSUPPORTED.  The cuts act on the row after guidance, bias,
 * penalties, DRY and the grammar mask; log-probs and last_logits stay on the raw head output.  The values are device data: one cached
 * step program serves any of them; cut calls replay step programs of their own, a call with all five NULL exactly the programs it ran
 * before.  Tokens do not depend on the number of lanes.  wrk_v7_generate_beam refuses them as it refuses every sampler.  The five
 * fields sit between poll_steps and num_top: every field behind them keeps its order, the filter fields last. */
#define WRK_MAX_STOP_TOKENS 16
#define WRK_MAX_STOP_SEQUENCES 8
#define WRK_MAX_STOP_SEQUENCE_LEN 8
#define WRK_STOP_TAIL_LEN 7
#define WRK_STOP_TAIL_EMPTY 0xFFFFFFFFu
#define WRK_STOP_MATCH_NONE 0xFFFFFFFFu
#define WRK_STOP_MATCH_TOKEN 0xFFFFFFFEu
typedef struct wrk_generate_options {
    const float *temperature, *top_p;
    const uint32_t *seed;
    const float *presence, *frequency, *decay;
    wrk_occurrence *occ;
    const wrk_logit_bias *bias;
    const uint32_t *bias_set;
    const float *guidance_scale;
    const uint32_t *guidance_first_tokens;
    const uint32_t *stop_tokens, *stop_offsets;
    uint32_t poll_steps;
    const float *top_n_sigma, *epsilon_cutoff, *eta_cutoff, *xtc_probability, *xtc_threshold;
    uint32_t num_top;
    float *out_logprob;
    uint32_t *out_top_ids;
    float *out_top_logprobs;
    wrk_token_window *window;
    const float *dry_multiplier, *dry_base;
    const uint32_t *dry_allowed_length, *no_repeat_ngram, *dry_breakers;
    uint32_t num_dry_breakers;
    const wrk_grammar *grammar;
    uint32_t *grammar_state;
    const uint32_t *stop_seq_tokens, *stop_seq_offsets, *stop_seq_owners;
    uint32_t *out_stop_match;
    uint32_t *stop_tail;
    const float *mirostat_tau, *mirostat_eta;
    float *mirostat_mu;
    const float *typical_p;
    const uint32_t *top_k;
    const float *min_p;
} wrk_generate_options;
int32_t wrk_v7_generate_stop(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                             uint32_t steps, const wrk_generate_options* opt, uint32_t* out_tokens, uint32_t* out_lengths,
                             float* last_logits_or_null, uint32_t* steps_run, float* elapsed_ms_or_null, uint32_t mode);
/* One counted draw of the stop-sequence matcher on the device, for num_rows owners: what a stop-sequence step program does with a drawn
 * token, and what a host-driven loop calls after each of its own draws.  Row r has the stop sequences of wrk_generate_options' three
 * arrays (num_rows + 1 owners entries; all three required), optionally the stop set stop_tokens[stop_offsets[r] .. stop_offsets[r + 1])
 * (both NULL: none), the tail tails[r][WRK_STOP_TAIL_LEN] (host u32, in/out) and the drawn token tokens[r].  out_match[r] (host u32
 * [num_rows]) receives WRK_STOP_MATCH_NONE, WRK_STOP_MATCH_TOKEN or the index of the matching stop sequence, resolved as in
 * wrk_generate_options; the tail then takes the token in, match or not.  Every id, token and non-EMPTY tail entry must be < num_vocab
 * (else WRK_E_ARG, as for the other errors listed there).  Blocking. */
int32_t wrk_stop_sequences_advance(wrk_ctx* ctx, uint32_t num_vocab, uint32_t num_rows, const uint32_t* stop_seq_tokens,
                                   const uint32_t* stop_seq_offsets, const uint32_t* stop_seq_owners, const uint32_t* stop_tokens,
                                   const uint32_t* stop_offsets, uint32_t* tails, const uint32_t* tokens, uint32_t* out_match);

/* A request queue in the decode loops: num_requests requests of different prompt and reply lengths are served on the num_batch slots of
 * `state` in one call, with the slot bookkeeping on the device (the reference's examples/batch.rs: "multiple inferences of different
 * length at the same time").  Request r has the prompt prompt_tokens[prompt_offsets[r] .. prompt_offsets[r + 1]) (CSR, at least one
 * token), max_new[r] >= 1, the stop set stop_tokens[stop_offsets[r] .. stop_offsets[r + 1]) (CSR, at most WRK_MAX_STOP_TOKENS ids; both
 * arrays NULL: no stops) and, per the pick, temperature / top_p / seed [r] and presence / frequency / decay [r].  The pick is one for the
 * call, as in wrk_generate_options: no sampler arrays: arg-max; sampler arrays: wrk_v7_generate_sample's; `occ` and the penalty arrays
 * (then the sampler arrays are required): wrk_v7_generate_penalized's on slot b's row of `occ`.
 * Requests are dispatched in index order: at step 0 request b goes to slot b (b < min(num_batch, num_requests)); slots that end in the
 * same step take the next requests in ascending slot order.  A slot that holds request r feeds p_0 .. p_{n-1} on consecutive steps; the
 * draws of the first n - 1 of them are discarded (not counted in the occurrence row, not checked against the stop set, no sampler step).
 * The draw of the step that feeds p_{n-1} is reply token y_0; from then on the slot feeds its own draws.  The sampler step of y_j is j:
 * u = SplitMix64((seed[r] << 32) | j), so a reply does not depend on when the request was scheduled.  The request ends at the first j
 * with y_j in its stop set (reason 1; the stop token is part of the reply), else at j + 1 == max_new[r] (reason 2).  A request still
 * running when max_steps steps have run has reason 3 and the tokens drawn so far; one never dispatched has reason 0 and length 0.
 * The step that ends a request resets its slot: the state slot to zeros (what wrk_v7_state_create leaves), or to a copy of init_state
 * (a buffer of exactly one sequence's state in wrk_v7_state_read's layout: one shared prefix for every request); with penalties the
 * slot's occurrence row to count 0 and no present bits -- banned bits are kept.  Then the slot takes the next request, or with none left
 * idles on its last token.  Every slot that starts a request at step 0 is reset the same way: the call does not continue from what the
 * slots held.  After the call the contents of the state slots and of rows [0, num_batch) of `occ` are unspecified.
 * The host submits steps in blocks of poll_steps (0: the default) and stops once every request has ended or max_steps have run:
 * *steps_run <= (ceil(needed / poll_steps) + 2) * poll_steps.  The requests are passed to the step program as data: one cached
 * program serves any queue (queue programs never share a program with the other loops).
 * Results, host u32 [num_requests]: lengths, reasons, slots, start_steps (the step that fed p_0); out_tokens: the reply of request r at
 * out_tokens[o_r .. o_r + lengths[r]), o_r = max_new[0] + .. + max_new[r - 1]; *steps_run.
 * WRK_E_ARG before any launch on: NULL opt / out or a NULL required array, num_requests == 0, an empty prompt, max_new == 0, offsets that
 * do not start at 0 or decrease, a token or stop id >= num_vocab, more than WRK_MAX_STOP_TOKENS stop ids for a request, sampler arrays
 * only partly given, penalty arrays without a table, a table with fewer slots than num_batch or of another vocabulary or context,
 * init_state of another size, max_steps == 0, and whatever wrk_v7_generate_stop rejects for the same pick.  mode bits 8-15 > 1 (lanes):
 * WRK_E_UNSUPPORTED -- a queue shared by several streams would need cross-stream atomics.
 * top_k / min_p [num_requests] (either may be NULL: off): request r's draws are wrk_sample_logits_filtered's, as in wrk_generate_options.
 * Log-probs, as in wrk_generate_options: on iff out_logprob is non-NULL (then, with num_top > 0, out_top_ids and out_top_logprobs are
 * required; all three NULL: off; anything else, or num_top > WRK_MAX_TOP_LOGPROBS: WRK_E_ARG).  The rows of a request's reply are cut
 * out of the step rows exactly as its tokens are: reply token j of request r has out_logprob[o_r + j] and out_top_ids /
 * out_top_logprobs[(o_r + j) * num_top ..], as wrk_top_logprobs gives them on the head output y_j was drawn from.  The rows of steps that
 * feed prompt tokens are discarded (prompt log-probs: wrk_v7_score).  out_logprob: host f32 [sum of max_new]; out_top_ids /
 * out_top_logprobs: host [sum of max_new][num_top].  They sit with the options, before the filter fields, as in wrk_generate_options:
 * wrk_queue_result keeps its six arrays.
 * mirostat_tau / mirostat_eta / typical_p [num_requests], as in wrk_generate_options: request r's draws are wrk_sample_logits_mirostat's
 * or wrk_sample_logits_typical's with its own parameters.  mirostat_mu (host f32 [num_requests], in/out, may be NULL): request r starts
 * from mirostat_mu[r] (NULL: 2 tau[r]) when it is dispatched, at step 0 or at a refill on the device -- never from what its slot's
 * previous request left -- and only its reply draws move it: the draws of the steps that feed prompt tokens are discarded for mu as
 * they are for the occurrence row.  On return entry r holds the mu after the request's reply draws for reasons 1, 2 and 3, and is
 * untouched for reason 0.  A reply and its final mu do not depend on the slot or the step the request was scheduled at.  mu is not part
 * of a state-pool entry: a session carries it through this array.
 * grammar / grammar_state (host u32 [num_requests], in/out, may be NULL), as in wrk_generate_options: one automaton for the call;
 * request r starts in grammar_state[r] (NULL: 0) when it is dispatched, at step 0 or at a refill on the device -- never in what its
 * slot's previous request left -- and only its reply draws move the state: the steps that feed prompt tokens do not.  On return entry
 * r holds the state after the request's reply draws for reasons 1, 2 and 3 (3: the state reached so far) and is untouched for reason
 * 0.  Requests that need different grammars use disjoint state sets of one automaton.  The state is not part of a state-pool entry: a
 * session carries it through this array.
 * Stop sequences, as in wrk_generate_options: stop_seq_owners has num_requests + 1 entries and request r owns stop sequences
 * [stop_seq_owners[r] .. stop_seq_owners[r + 1]).  Only reply draws enter a request's tail: prompt tokens and the discarded draws of
 * the steps that feed them never do, so a prompt that is (or ends in the beginning of) a stop sequence does not end its reply.  The
 * tail starts empty when the request is dispatched, at step 0 or at a refill on the device -- never with what its slot's previous
 * request left -- and is not returned.  A match ends the request with reason 1 exactly as a stop token does: the slot resets and
 * refills in the same step and a pool entry is saved as for a stop token.  out_stop_match (host u32 [num_requests], may be NULL):
 * WRK_STOP_MATCH_NONE for reasons 0, 2 and 3, else as in wrk_generate_options.  The tail is not part of a state-pool entry.  The four
 * fields sit between grammar_state and mirostat_tau.
 * DRY and the n-gram ban, as in wrk_generate_options: `window` has at least num_batch slots and slot b serves whatever request runs
 * on state slot b; dry_multiplier / dry_base / dry_allowed_length / no_repeat_ngram are per request [num_requests], the breakers are
 * call-wide.  A slot's window is set to length 0 when a request is dispatched to it, at step 0 or at a refill on the device, and
 * takes only that request's reply draws: prompt tokens and the discarded draws of the steps that feed them never enter it.  After
 * the call rows [0, num_batch) of the window are unspecified.  The window is not part of a state-pool entry.  The seven fields sit
 * between out_top_logprobs and grammar.
 * Prompt intake.  prompt_context_from (host u32 [num_requests], NULL: off -- everything above) lets a request's prompt enter its slot's
 * context, the slot's occurrence row and its window: with f = prompt_context_from[r] the tokens p_f .. p_{n-1} enter in order, on the
 * device, after the reset (or the restore from a history pool) that the dispatch makes and before the row y_0 is picked from is
 * penalised; f >= n: none.  A token enters the occurrence row as wrk_occurrence_add does with decay[r] (every count *= decay[r], then
 * count[p] += w[p], present[p] = 1) and the window as wrk_token_window_add does (a full ring drops its oldest token).  The draws of the
 * steps that feed prompt tokens stay discarded, and mu, the automaton state, the stop tail and the log-probs see what they saw: a reply
 * still does not depend on when or where its request was scheduled.  An offset, not a flag: a state-pool entry has consumed its
 * conversation but the last reply token, which therefore opens the next turn's prompt and which the entry's history has already
 * counted as a draw -- such a turn passes 1.  WRK_E_ARG before any launch: prompt_context_from with neither `occ` (and its penalty
 * arrays) nor `window`.  The offsets are device data: one cached step program serves any of them; intake calls replay step programs of
 * their own, a call with NULL exactly the programs it ran before.  `history` (NULL: off) is the history pool of a call with a state
 * pool, described with wrk_queue_pool below; without a pool (wrk_v7_generate_queue) it is WRK_E_ARG.  The two fields sit between
 * max_steps and num_top: every field behind them keeps its order, the filter fields last.
 * Logit bias, as in wrk_generate_options: one object for the call, bias_set per request (host u32 [num_requests]; NULL: set 0 for
 * every request).  Request r's rows are biased with set bias_set[r] from the step it is dispatched, at step 0 or at a refill on the
 * device, and never with what its slot's previous request used; the rows of the steps that feed prompt tokens are biased too, their
 * draws are discarded as before.  A reply does not depend on the slot or the step the request was scheduled at.  Nothing of the bias
 * belongs to a state-pool or history-pool entry.  The two fields sit directly behind `occ`.
 * Guidance (wrk_generate_options) is not taken through these options: a refilled slot's partner needs the new request's negative prompt,
 * which wrk_v7_generate_queue_guided (below) takes.  guidance_scale non-NULL is WRK_E_UNSUPPORTED before any launch in
 * wrk_v7_generate_queue and wrk_v7_generate_queue_pool; the field sits directly behind `bias_set`. */
typedef struct wrk_history_pool wrk_history_pool;   /* a history pool beside a state pool: wrk_queue_pool, below */
typedef struct wrk_queue_options {
    uint32_t num_requests;
    const uint32_t *prompt_tokens, *prompt_offsets, *max_new;
    const uint32_t *stop_tokens, *stop_offsets;
    const float *temperature, *top_p;
    const uint32_t *seed;
    const float *presence, *frequency, *decay;
    wrk_occurrence *occ;
    const wrk_logit_bias *bias;
    const uint32_t *bias_set;
    const float *guidance_scale;
    const wrk_buf *init_state;
    uint32_t poll_steps, max_steps;
    const uint32_t *prompt_context_from;
    wrk_history_pool *history;
    uint32_t num_top;
    float *out_logprob;
    uint32_t *out_top_ids;
    float *out_top_logprobs;
    wrk_token_window *window;
    const float *dry_multiplier, *dry_base;
    const uint32_t *dry_allowed_length, *no_repeat_ngram, *dry_breakers;
    uint32_t num_dry_breakers;
    const wrk_grammar *grammar;
    uint32_t *grammar_state;
    const uint32_t *stop_seq_tokens, *stop_seq_offsets, *stop_seq_owners;
    uint32_t *out_stop_match;
    const float *mirostat_tau, *mirostat_eta;
    float *mirostat_mu;
    const float *typical_p;
    const uint32_t *top_k;
    const float *min_p;
} wrk_queue_options;
typedef struct wrk_queue_result {
    uint32_t *lengths, *reasons, *slots, *start_steps, *out_tokens, *steps_run;
} wrk_queue_result;
int32_t wrk_v7_generate_queue(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                              const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode);

/* A state pool under the queue: sessions across calls, and several requests from one prefix.  `states` holds num_entries states, entry k at
 * float offset k * L * (S+2) * D in wrk_v7_state_read's layout (what init_state holds), so wrk_buf_copy / wrk_buf_read / wrk_buf_write
 * with that offset move entries to and from snapshots and the host.  start / save: host u32 [num_requests], WRK_QUEUE_NO_ENTRY for none;
 * either array may be NULL (all none).  Request r with start[r] = k begins from a copy of entry k (at step 0 or at a refill), one with
 * none as wrk_v7_generate_queue's: from zeros or init_state.  When request r ends with reason 1 or 2 and save[r] = k, entry k receives
 * the slot's state in the step that ends it, on the device: the state has consumed the prompt and y_0 .. y_{j-1}, the last reply token
 * y_j is not fed -- what wrk_v7_generate_stop freezes for a sequence that ends there.  Reasons 3 and 0 write nothing: the entry keeps its
 * bits.  saved (host u32 [num_requests], may be NULL): 1 iff the entry was written.  start[r] == save[r] (a session in place) and any
 * number of requests reading an entry that nobody saves are allowed.  WRK_E_ARG before any launch, besides wrk_v7_generate_queue's: a NULL
 * pool or `states`, an index >= num_entries, a buffer whose size is not num_entries states or of another context, `states` the same
 * buffer as init_state, two requests saving to one entry, a request reading an entry that another request of the call saves to.
 * WRK_E_UNSUPPORTED: (S+2) * D not a multiple of 4.  The pool's address and entry count are data of the step program: one cached
 * program serves any pool, and pool programs never share a program with wrk_v7_generate_queue's.  Occurrence rows are reset at every
 * request start, as without a pool -- unless the call has a `history` (below).
 * A history pool beside the state pool: what a conversation's penalties have seen, kept on the device next to its state.  Entry k of a
 * wrk_history_pool holds an occurrence row -- count f32 [num_vocab] and the present bit per token -- and, with window_capacity > 0, a
 * token window (the ring, its length and its write position): what slot b of a wrk_occurrence and of a wrk_token_window hold.  Banned
 * bits are not part of an entry: they stay the slot's, as at a reset.  create: empty entries (zero counts, no bits, empty windows).
 * load: entry <- counts / present (host f32 / u32 [num_vocab], both or neither: an empty row; counts finite, present 0 or 1) and
 * tokens[0..n) (n <= window_capacity, ids < num_vocab, oldest first; NULL: an empty window).  back: the reverse; tokens_out host u32
 * [window_capacity] (may be NULL without windows), *len the window's length.  put: entry <- slot `batch` of `occ` (the present bit
 * only) and of `window`; get: slot <- entry, the slot keeping its banned bits; both on the device, with the copy kernel of the queue's
 * turnover.  occ or window may be NULL (one is required); a pool with windows needs `window`, of the pool's capacity, and a pool
 * without them takes none; context and num_vocab must be the pool's (else WRK_E_ARG).  All six are blocking.
 * wrk_queue_options.history (NULL: off; wrk_queue_pool keeps its five fields, so the pointer travels with the options of the call):
 * entry k of it belongs to entry k of `states`, and start / save index both.  Request r with
 * start[r] = k begins, at step 0 or at a refill, with slot.count = entry.count, slot.flags = (slot.flags & banned) | entry.present and
 * the entry's window, order and length kept; a request with no start entry begins as without a history -- row reset, bans kept,
 * window empty.  When r ends with reason 1 or 2 and save[r] = k, entry k receives the slot's row (the present bit only) and window in
 * the step that ends r, on the device, after that step's counted draw: the entry has counted the last reply token y_j that the saved
 * state has not consumed -- what wrk_v7_generate_stop leaves in the handles of a sequence that ends there.  Reasons 3 and 0 write
 * nothing; saved[r] speaks for both pools.  prompt_context_from enters its tokens after the restore.  WRK_E_ARG before any launch,
 * nothing on the device changed: a history in a call without a pool; a history with neither `occ` nor `window` in the options; a history of another context, num_vocab or
 * num_entries; a history with windows of another capacity than `window`'s; `window` with a history created without windows; a history
 * with windows and no `window`.  The pool's addresses are device data: one cached step program serves any history pool; history calls
 * replay step programs of their own, a call with NULL exactly the programs it ran before. */
#define WRK_QUEUE_NO_ENTRY 0xFFFFFFFFu
int32_t wrk_history_pool_create(wrk_ctx* ctx, uint32_t num_entries, uint32_t num_vocab, uint32_t window_capacity, wrk_history_pool** out);
int32_t wrk_history_pool_destroy(wrk_history_pool* history);
int32_t wrk_history_pool_load(wrk_ctx* ctx, wrk_history_pool* history, uint32_t entry, const float* counts_or_null,
                              const uint32_t* present_or_null, const uint32_t* tokens_or_null, uint32_t n);
int32_t wrk_history_pool_back(wrk_ctx* ctx, const wrk_history_pool* history, uint32_t entry, float* counts, uint32_t* present,
                              uint32_t* tokens_out, uint32_t* len);
int32_t wrk_history_pool_put(wrk_ctx* ctx, wrk_history_pool* history, uint32_t entry, wrk_occurrence* occ_or_null, uint32_t batch,
                             wrk_token_window* window_or_null);
int32_t wrk_history_pool_get(wrk_ctx* ctx, wrk_history_pool* history, uint32_t entry, wrk_occurrence* occ_or_null, uint32_t batch,
                             wrk_token_window* window_or_null);
typedef struct wrk_queue_pool {
    wrk_buf *states;
    uint32_t num_entries;
    const uint32_t *start, *save;
    uint32_t *saved;
} wrk_queue_pool;
int32_t wrk_v7_generate_queue_pool(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                   const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_pool* pool);

/* Guidance in the request queue: every request brings its own negative prompt and scale, and a refilled slot's partner takes the new
 * request's negative prompt in at decode rate beside it.  wrk_v7_generate_queue with classifier-free guidance (wrk_guide_logits).
 * Layout.  A guided queue of B = num_batch request slots runs on a state of at least 2 B slots; request slot b is the pair (state slot b,
 * state slot B + b): the conditional half and its partner.  B <= 128: the 2 B slot records fit the one workgroup of the advance kernel.
 * A request.  Request r has the prompt p_0 .. p_{n-1} of wrk_queue_options (n >= 1), the negative prompt q_0 .. q_{m-1} =
 * negative_tokens[negative_offsets[r] .. negative_offsets[r + 1]) (CSR, m >= 0) and the scale s = scale[r], finite and >= 0.  m == 0 is
 * allowed only with s == 1: an unguided request inside a guided queue, whose partner slot idles.  Let L = max(n, m).
 * Dispatch.  The order is wrk_v7_generate_queue's: index order, ascending slot order among pairs that end in the same step.  A pair
 * given request r at step f (f = 0, or the step after the one that ended the pair's previous request) feeds p_0 at step f + L - n and
 * q_0 at step f + L - m, so both halves feed their last prompt token at step f + L - 1.  The draw of that step, made on the guided row,
 * is reply token y_0; from then on both halves feed the same draws.  The sampler step of y_j is j (the step base is f + L - 1), and
 * start_steps[r] stays "the step that fed p_0" = f + L - n: reply token j of request r was drawn by step start_steps[r] + n - 1 + j, as
 * without guidance.  The schedule is a pure function of (n, m, reply lengths); with every m <= n it is wrk_v7_generate_queue's.
 * The wait.  The half that starts late waits until its first token: it feeds a valid id, its draws are ignored, and nothing is
 * counted, matched or pushed for it.  The state slot of a half is set to its start state by the step program directly in front of the
 * step that feeds that half's first token -- for a half that starts at f this is wrk_v7_generate_queue's reset; an idle or waiting slot
 * still runs the model on its state, so a half that starts late is reset when it starts, not when the pair is dispatched.  The start
 * state is zeros, or init_state (wrk_queue_options) for the conditional half and negative_init_state for the partner, both one shared
 * prefix state in wrk_v7_state_read's layout.  The pair's pick rows -- sampler, filter, Mirostat / typical, automaton state, bias set,
 * DRY values, stop tail, penalty values, the occurrence reset, the window reset, the scale -- are the conditional request's and are
 * written by the dispatch; no draw counts before y_0, so nothing observes when within [f, f + L - 1] they are written.  A partner
 * with m == 0 is neither reset nor fed.
 * End.  The conditional half decides the end -- stop id, stop sequence or max_new; reasons 1, 2, 3 and 0 as in wrk_v7_generate_queue.
 * Both halves are released in that step and the pair takes the next request in the same step.  A request that was given to a pair but
 * whose p_0 was not fed when max_steps ran out has reason 0.
 * The guided row is wrk_guide_logits' row of the pair's two head rows with the pair's scale, bit for bit; the scale is data of the step
 * program, written by the dispatch.  A pair with s == 1 passes its conditional row through as words and does not read the partner row.
 * Log-probs stay on the raw conditional rows.  Order within a step: as wrk_generate_options' guidance.
 * Composition: every sampler family, top_k / min_p, mirostat_mu per request, penalties with prompt_context_from (the conditional prompt
 * only), DRY / the n-gram window, grammar, logit bias, stop ids and stop sequences, log-probs, max_steps and poll_steps -- `occ`, `window`
 * and every per-slot row are num_batch wide.  Not built: a state pool or a history pool under a guided queue (no entry point takes
 * both; opt->history is WRK_E_ARG), lanes (mode bits 8-15 > 1: WRK_E_UNSUPPORTED), scales that change along a reply, negative prompts
 * through the prefill GEMMs.
 * WRK_E_ARG before any launch, besides wrk_v7_generate_queue's cases: a NULL `guide`, `scale` or `negative_offsets`; offsets that do
 * not start at 0 or decrease; negative_tokens NULL with a non-empty negative prompt; a scale that is NaN, infinite or negative; an empty
 * negative prompt with a scale != 1; a negative token >= num_vocab; a state of fewer than 2 * num_batch slots; num_batch > 128;
 * negative_init_state of another size or context, or the same buffer as init_state; opt->guidance_scale non-NULL (the scales come from
 * `guide`).  The requests, negative prompts and scales are data of the step program: one cached program serves any guided queue;
 * guided queue programs never share a program with the other loops, and a call without this entry point replays exactly the programs
 * it replayed before. */
typedef struct wrk_queue_guidance {
    const float *scale;
    const uint32_t *negative_tokens;
    const uint32_t *negative_offsets;
    const wrk_buf *negative_init_state;
} wrk_queue_guidance;
int32_t wrk_v7_generate_queue_guided(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                     const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_guidance* guide);

/* The cuts of wrk_sample_logits_cut in the request queue.  wrk_queue_options keeps its fields, so the five arrays travel beside it, as the
 * guidance does: top_n_sigma / epsilon_cutoff / eta_cutoff / xtc_probability / xtc_threshold (host f32 [num_requests], any may be NULL:
 * off; the two XTC arrays both or neither), validated as in wrk_generate_options.  Request r's reply draws are wrk_sample_logits_cut's
 * with its own values and its top_k / min_p; the values are written into the slot's row by the dispatch, at step 0 on the host and at a
 * refill on the device, and the coin of reply token j is a pure function of (seed[r], j): a reply does not depend on the slot or the
 * step the request was scheduled at, and a slot in its prompt phase draws no coin that matters.  `pool` non-NULL: the call is
 * wrk_v7_generate_queue_pool's with that pool; `guide` non-NULL: wrk_v7_generate_queue_guided's with that guidance; both NULL:
 * wrk_v7_generate_queue's; both set: WRK_E_ARG (no entry point takes both).  Everything else -- arguments, results, errors -- is the
 * selected call's.  WRK_E_ARG before any launch, besides that call's: a NULL `cuts`, the cuts without the sampler arrays or together
 * with mirostat_* or typical_p, the values wrk_sample_logits_cut rejects.  With all five arrays NULL the call replays exactly the
 * programs of the selected call. */
typedef struct wrk_queue_cuts {
    const float *top_n_sigma, *epsilon_cutoff, *eta_cutoff, *xtc_probability, *xtc_threshold;
    const wrk_queue_pool *pool;
    const wrk_queue_guidance *guide;
} wrk_queue_cuts;
int32_t wrk_v7_generate_queue_cut(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                  const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_cuts* cuts);

/* Beam search in the decode loops (Hugging Face's num_beams, vLLM's beam_search): the search over continuations that the other loops do
 * not make.  A hypothesis of an RWKV model is one fixed-size state slot, so a beam step is the batched step, a selection over at most
 * W * W + W candidates per group, and a device-to-device permutation of state slots -- all inside the captured step program.
 * Slots.  G groups of W = num_beams beams run on B = G * W consecutive state slots, 1 <= W <= WRK_MAX_BEAMS and B <= the state's
 * num_batch; group g owns slots gW .. gW + W - 1.  A slot carries score (f32 sum of log-probs), key (what it is ordered by), length
 * (generated tokens) and a status WRK_BEAM_LIVE / WRK_BEAM_DONE / WRK_BEAM_DEAD.
 * Start.  Slot gW is LIVE with score 0, length 0 and the caller's state (what wrk_v7_infer or a previous call left there); the group's
 * other slots are DEAD and their contents are overwritten.  Every slot of the group feeds first_tokens[g].
 * One step, after the layers and the head, on the row the pick of wrk_generate_options would see: the head output, or with a logit bias
 * the biased row (set bias_set[g] for every slot of group g), so log-probs, ties and bans follow that row.
 *   1. Every LIVE slot b gives W candidates: its W first tokens t_{b,j} in wrk_sample_logits' order with log-probs lp_{b,j}, bit for bit
 *      what wrk_top_logprobs returns for the row with num_top = W (same rows, num_vocab and stride).  A token whose lp is -inf or NaN is
 *      no candidate.  Candidate (b, j): raw = score_b + lp_{b,j} (one f32 addition), len = length_b + 1, key = raw * inv_norm[len] (one
 *      f32 multiplication), inv_norm[l] = (float)(1.0 / pow((double)l, (double)length_penalty)) computed once per call on the host; with
 *      length_penalty 0 key == raw bit for bit.  No transcendental runs on the device in the selection.
 *   2. Every DONE slot gives one candidate, itself, with the key it got when it ended.
 *   3. The group's candidates are ordered by key descending, ties by slot of origin ascending, then j ascending; the first W survive
 *      (fewer if there are fewer).
 *   4. A surviving DONE slot stays where it is (nothing is copied, its frozen snapshot stays valid); the group's other slots, ascending,
 *      take the surviving live candidates in their order; slots left over become DEAD with score and key -inf and length 0.
 *   5. A live candidate (p, j) placed in slot q: state_q <- the post-step state of slot p (no bytes move when p == q; a slot may be source
 *      and destination in one step: swaps, chains and broadcasts are all correct), score_q = raw, key_q = key, length_q = len, and the
 *      slot feeds t_{p,j} next.  It is DONE if t_{p,j} is in the group's stop set (stop_tokens / stop_offsets: a CSR per group of G + 1
 *      offsets, at most WRK_MAX_BEAM_STOP_TOKENS ids: a group's set is kept sorted and searched, so it may be larger than a sequence's
 *      WRK_MAX_STOP_TOKENS), else LIVE.  A slot that became DONE is snapshotted in that step, state only: its state
 *      has consumed everything but its last token, as a sequence wrk_v7_generate_stop froze.
 *   6. The step records step_tokens[s][q] and step_parents[s][q] (a slot index) and step_scores[s][q] (score_q after the step).  A slot
 *      not filled in the step (a staying DONE slot, a DEAD one) records WRK_BEAM_NO_TOKEN and parent q.  DONE and DEAD slots go on
 *      feeding a valid token; what the steps do to their live state does not matter.
 * End.  A group is over when it has no LIVE slot.  The host submits steps in blocks of poll_steps (0: the default) and stops once every
 * group is over, or after `steps` steps; DONE slots are then restored from their snapshots.  A group's hypotheses are its non-DEAD
 * slots by key descending, ties by slot (a LIVE slot's key is score * inv_norm[length]).  wrk_beam_result, all host arrays: per group g
 * and rank r at [g * W + r]: lengths, scores, finished (1: DONE) and slots, WRK_BEAM_NO_TOKEN in slots and 0 elsewhere for a rank
 * the group does not have; tokens [G][W][steps]: the rank's tokens (the stop token included), backtracked through step_parents on the
 * host; num_hyps [G]; *steps_run.  step_tokens / step_parents (u32) and step_scores (f32), [steps][B], may each be NULL; rows at or
 * after *steps_run are not written.  After the call slot slots[g * W + r] holds that hypothesis's state, having consumed everything but
 * its last token: the next turn's prompt begins with that token.  The contents of DEAD slots are unspecified.
 * Composition.  `gen` (may be NULL) carries what the call shares with wrk_generate_options: stop_tokens / stop_offsets, bias / bias_set
 * (one set word per group; NULL: set 0) and poll_steps.  Every other field of it must be NULL / 0: a call that passes a sampler,
 * penalties, DRY, a grammar, stop sequences or log-probs is refused, as is one with lanes (bits 8-15 of mode above 1); penalties, DRY
 * and a grammar per hypothesis come through wrk_v7_generate_beam_context below.  W = 1 is greedy
 * decoding with a score.  WRK_E_ARG before any launch: a NULL opt / out or a NULL required array (every array of wrk_beam_result but
 * the three step arrays), num_beams outside [1, WRK_MAX_BEAMS], G * W above the state's num_batch or above 256, a length_penalty that
 * is negative, infinite or NaN or so large that inv_norm[steps] is not a normal number, a first token or stop id >= num_vocab, steps
 * == 0, and the stop-set and bias errors of wrk_generate_options (a group's cap being WRK_MAX_BEAM_STOP_TOKENS).  num_vocab > 2^20: WRK_E_UNSUPPORTED.  The slot records, inv_norm,
 * the stop sets and W are device data: one cached step program per (state, B) serves any of them; beam calls replay step programs
 * of their own, every other call exactly the programs it ran before. */
#define WRK_MAX_BEAMS 16
#define WRK_MAX_BEAM_STOP_TOKENS 128
#define WRK_BEAM_NO_TOKEN 0xFFFFFFFFu
#define WRK_BEAM_NO_COPY 0xFFFFFFFFu
enum { WRK_BEAM_DEAD = 0, WRK_BEAM_LIVE = 1, WRK_BEAM_DONE = 2 };
typedef struct wrk_beam_options {
    uint32_t num_beams;
    float length_penalty;
    const wrk_generate_options *gen;
} wrk_beam_options;
typedef struct wrk_beam_result {
    uint32_t *tokens, *lengths;
    float *scores;
    uint32_t *finished, *slots, *num_hyps, *steps_run;
    uint32_t *step_tokens, *step_parents;
    float *step_scores;
} wrk_beam_result;
int32_t wrk_v7_generate_beam(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_groups,
                             uint32_t steps, const wrk_beam_options* opt, const wrk_beam_result* out, float* elapsed_ms_or_null, uint32_t mode);
/* Beam search with a context per hypothesis (Hugging Face's no_repeat_ngram_size and repetition_penalty under num_beams, constrained beam
 * search): wrk_v7_generate_beam with one more argument.  A wrk_beam_context holds any subset of: an occurrence table with presence /
 * frequency / decay (decay NULL: 1), a token window with the dry_* / no_repeat_ngram arrays and the breakers, a grammar with start
 * states.  Every array holds one value per group [G], as bias_set does; table and window have at least G * W slots, slot q of the call
 * using slot q of each.
 * Start.  Slot gW carries the caller's context -- what wrk_occurrence_add / _ban and wrk_token_window_add left in slot gW of the table
 * and the window, and grammar_state[g] -- and the context rows of the group's other slots are overwritten, as their states are.
 * One step, on the row the pick would see and in the order of the other loops' chain:
 *   a. The row of slot b: head output -> bias -> penalties with slot b's occurrence row -> DRY / n-gram ban with slot b's window ->
 *      grammar mask with slot b's automaton state: bit for bit what wrk_penalize_logits, wrk_dry_logits and wrk_constrain_logits give.
 *   b. Steps 1 - 6 above run on that row, so scores are sums of log-probs under the modified row.  A LIVE slot whose row has no finite
 *      log-prob gives no candidate and dies.
 *   c. The context follows the hypothesis: for every slot q that step 5 gives the state of another slot p, slot q's occurrence row
 *      (counts and both flag bits: bans follow the hypothesis), window (ring and the two meta words) and automaton state become slot
 *      p's of before the step.  Every source is read before any destination is written (swaps, chains, broadcasts); other slots move no
 *      bytes.
 *   d. Every slot filled in the step (step_tokens is not WRK_BEAM_NO_TOKEN; LIVE or DONE) then counts the token it was given in its own
 *      context: the occurrence update with the group's decay, the automaton advance, the window push.  Two children of one parent each
 *      count only their own token.  Slots not filled (a staying DONE slot, a DEAD one) are not touched, so a DONE slot keeps the context
 *      it ended with and needs no snapshot.
 * End.  Slot slots[g * W + r] holds that hypothesis's context beside its state; the context has the last token counted, which the state
 * has not consumed (as wrk_v7_generate_stop leaves a sequence).  out_grammar_state (may be NULL) [B]: the automaton state per slot.
 * WRK_E_ARG before any launch, as wrk_generate_options: arrays without their table, window or grammar; a table, window or grammar of
 * another context or vocabulary; fewer than G * W slots; values out of range; a start state >= num_states.  What `gen` refuses in
 * wrk_v7_generate_beam it refuses here: samplers, stop sequences, log-prob rows, guidance, lanes -- and penalty, DRY or grammar fields
 * in `gen` itself.  ctx NULL or all-empty: wrk_v7_generate_beam, the same programs and bits.  num_beams = 1: the greedy call with the
 * same context.  Context calls replay step programs of their own (the kinds' key bits). */
typedef struct wrk_beam_context {
    wrk_occurrence* occ;
    const float *presence, *frequency, *decay;
    wrk_token_window* window;
    const float *dry_multiplier, *dry_base;
    const uint32_t *dry_allowed_length, *no_repeat_ngram, *dry_breakers;
    uint32_t num_dry_breakers;
    const wrk_grammar* grammar;
    const uint32_t* grammar_state;
    uint32_t* out_grammar_state;
} wrk_beam_context;
int32_t wrk_v7_generate_beam_context(wrk_ctx* ctx, wrk_v7_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_groups,
                                     uint32_t steps, const wrk_beam_options* opt, const wrk_beam_result* out, float* elapsed_ms_or_null,
                                     uint32_t mode, const wrk_beam_context* context);
/* The context's half of wrk_v7_state_permute, for a host-driven loop (wrk_beam_step + wrk_v7_state_permute + these): slot q of the table
 * / the window <- slot parents[q] for q in [0, n) -- counts and flags / ring and meta -- every slot read before any is written.  Slots
 * with parents[q] == q move no bytes and slots >= n are untouched.  parents: host u32 [n], each < n; n <= num_batch (else WRK_E_ARG).
 * Blocking. */
int32_t wrk_occurrence_permute(wrk_ctx* ctx, wrk_occurrence* occ, const uint32_t* parents, uint32_t n);
int32_t wrk_token_window_permute(wrk_ctx* ctx, wrk_token_window* window, const uint32_t* parents, uint32_t n);
/* One beam step on rows of f32 logits, for a host-driven loop: steps 1 - 5 above on logits [num_groups * num_beams][row_stride] (first
 * num_vocab used; a caller with a bias applies wrk_bias_logits first).  scores / keys (host f32) and lengths / status (host u32), all
 * [B], in/out: the slot records; stop_tokens / stop_offsets: the groups' stop sets (both NULL: none).  Out, host u32 [B]: out_tokens
 * (the token the slot feeds next, WRK_BEAM_NO_TOKEN for a slot not filled), out_parents (slot indices) and out_copy_src, the step's copy
 * list: slot q takes the state of slot out_copy_src[q], WRK_BEAM_NO_COPY for a slot that moves no bytes -- wrk_v7_state_permute's
 * argument once NO_COPY entries are replaced by q.  inv_norm is computed for the lengths the records reach.  WRK_E_ARG: NULL arrays, W
 * out of range, B > 256, a status above WRK_BEAM_DONE, a bad length_penalty, a stop id >= num_vocab, and what wrk_top_logprobs
 * rejects.  Blocking. */
int32_t wrk_beam_step(wrk_ctx* ctx, const wrk_buf* logits, uint32_t num_vocab, uint32_t row_stride, uint32_t num_groups, uint32_t num_beams,
                      float length_penalty, const uint32_t* stop_tokens, const uint32_t* stop_offsets, float* scores, float* keys,
                      uint32_t* lengths, uint32_t* status, uint32_t* out_tokens, uint32_t* out_parents, uint32_t* out_copy_src);
/* state slot q <- state slot parents[q] for q in [0, n), all layers, on the device: every slot is read before any is written (a gather
 * into a scratch of n slots, then a scatter), so any map is correct -- swaps, chains, many-to-one.  Slots with parents[q] == q move no
 * bytes and slots >= n are untouched.  parents: host u32 [n], each < n; n <= the state's num_batch (else WRK_E_ARG).  Blocking. */
int32_t wrk_v7_state_permute(wrk_ctx* ctx, wrk_v7_state* state, const uint32_t* parents, uint32_t n);

/* ---------------------------------------------------------------- RWKV-6 (v6::Model, src/runtime/v6.rs)
 * Same chunk semantics, state layout ([D, S+2, B] per layer: v6.rs:150-214 == v7) and entry points as the V7
 * runner; one kernel per reference TensorOp (v6.rs:701-958), decode steps replayed from a hipGraph.
 * Every decode loop (generate_greedy ... generate_queue_pool) reads bits 0-7 of `mode` and runs on one lane: bits 8-15,
 * RWKV-7's number of concurrent pipelines, are ignored, except that a queue call refuses more than one lane
 * (WRK_E_UNSUPPORTED) as RWKV-7's does. */
typedef struct wrk_v6_model wrk_v6_model;

typedef struct wrk_v6_layer_desc {
    const wrk_buf *ln1_w, *ln1_b, *ln2_w, *ln2_b;               /* f16 [D] */
    const wrk_buf *time_decay;                                  /* f16 [D]                        (v6.rs:1051) */
    const wrk_buf *time_first;                                  /* f32 [D] = [S, H]               (v6.rs:1052, load_vector_f32) */
    const wrk_buf *time_mix_x;                                  /* f16 [D] */
    const wrk_buf *time_mix;                                    /* f16 [D, 1, 5] = w, k, v, r, g  (v6.rs:1054-1071) */
    const wrk_matrix *time_decay_w1, *time_decay_w2, *time_mix_w1;
    const wrk_matrix *time_mix_w2[5];                           /* the batched [R, D, 5] matrix as five [R -> D] matrices */
    const wrk_matrix *w_k, *w_v, *w_r, *w_g, *w_o;
    const wrk_buf *gn_w, *gn_b;
    const wrk_buf *ffn_mix_k, *ffn_mix_r;
    const wrk_matrix *ffn_w_k, *ffn_w_v, *ffn_w_r;
} wrk_v6_layer_desc;

typedef struct wrk_v6_model_desc {
    uint32_t num_layer, num_emb, num_hidden, num_vocab, num_head;
    uint32_t time_mix, time_decay;                              /* v6::CustomInfo (v6.rs:53-59) */
    uint32_t rescale;                                           /* default 6 (v6.rs:49) */
    const wrk_buf *ln0_w, *ln0_b, *ln_out_w, *ln_out_b, *emb_f16;
    const wrk_matrix* head;
    const wrk_v6_layer_desc* layers;
} wrk_v6_model_desc;

int32_t wrk_v6_model_create(wrk_ctx* ctx, const wrk_v6_model_desc* desc, wrk_v6_model** out);
int32_t wrk_v6_model_destroy(wrk_v6_model* model);
size_t wrk_v6_model_token_bytes(const wrk_v6_model* model, uint32_t num_batch);
/* v6::Bundle::new state allocation; the handle type is shared with V7 (identical layout) */
int32_t wrk_v6_state_create(wrk_ctx* ctx, const wrk_v6_model* model, uint32_t num_batch, wrk_v7_state** out);
/* as wrk_v7_infer / wrk_v7_generate_greedy.  mode 1: jobs whose tokens are one per sequence (decode) run the fused
 * 7-launch layer (LN prologues in the consumer matvec, v6_mix / v6_head kernels, gated ffn epilogue); everything else,
 * and mode 0, runs one kernel per reference op (v6.rs:701-958) */
int32_t wrk_v6_infer(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state,
                     const uint32_t* tokens, const uint16_t* emb_rows, const uint32_t* cursors, uint32_t num_token,
                     const uint32_t* headers, uint32_t num_header, float* logits, uint32_t* argmax, uint32_t mode);
int32_t wrk_v6_generate_greedy(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state,
                               const uint32_t* first_tokens, uint32_t num_batch, uint32_t steps,
                               uint32_t* out_tokens, float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);
/* as wrk_v7_generate_sample */
int32_t wrk_v6_generate_sample(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                               uint32_t steps, const float* temperature, const float* top_p, const uint32_t* seed,
                               uint32_t* out_tokens, float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);
/* as wrk_v7_score */
int32_t wrk_v6_score(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state,
                     const uint32_t* tokens, const uint16_t* emb_rows, const uint32_t* cursors, uint32_t num_token,
                     const uint32_t* headers, uint32_t num_header, const uint32_t* targets, float* logprob, uint32_t* rank, uint32_t mode);

/* as wrk_v7_generate_penalized */
int32_t wrk_v6_generate_penalized(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                                  uint32_t steps, const float* temperature, const float* top_p, const uint32_t* seed, const float* presence,
                                  const float* frequency, const float* decay, wrk_occurrence* occ, uint32_t* out_tokens,
                                  float* last_logits_or_null, float* elapsed_ms_or_null, uint32_t mode);

/* as wrk_v7_generate_stop */
int32_t wrk_v6_generate_stop(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_batch,
                             uint32_t steps, const wrk_generate_options* opt, uint32_t* out_tokens, uint32_t* out_lengths,
                             float* last_logits_or_null, uint32_t* steps_run, float* elapsed_ms_or_null, uint32_t mode);

/* as wrk_v7_generate_queue */
int32_t wrk_v6_generate_queue(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                              const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode);
/* as wrk_v7_generate_queue_pool */
int32_t wrk_v6_generate_queue_pool(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                   const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_pool* pool);
/* as wrk_v7_generate_queue_guided */
int32_t wrk_v6_generate_queue_guided(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                     const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_guidance* guide);
/* as wrk_v7_generate_queue_cut */
int32_t wrk_v6_generate_queue_cut(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, uint32_t num_batch, const wrk_queue_options* opt,
                                  const wrk_queue_result* out, float* elapsed_ms_or_null, uint32_t mode, const wrk_queue_cuts* cuts);
/* as wrk_v7_generate_beam */
int32_t wrk_v6_generate_beam(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_groups,
                             uint32_t steps, const wrk_beam_options* opt, const wrk_beam_result* out, float* elapsed_ms_or_null, uint32_t mode);
/* as wrk_v7_generate_beam_context */
int32_t wrk_v6_generate_beam_context(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, const uint32_t* first_tokens, uint32_t num_groups,
                                     uint32_t steps, const wrk_beam_options* opt, const wrk_beam_result* out, float* elapsed_ms_or_null,
                                     uint32_t mode, const wrk_beam_context* context);

/* Parity instrumentation, as wrk_v7_infer_layer / wrk_v7_frame_read (RWKV-6 has no layer-0 value to carry):
 *   wrk_v6_infer_layer: run ONLY `layer` of a job on a caller-supplied layer input x (f16 [D, num_token]) and the state as it stands;
 *                       the launches are the ones wrk_v6_infer picks for these cursors and this mode (mode 1, one token per sequence:
 *                       the fused 7-launch layer, or the op list where it declines; mode 1 otherwise: the merged op list).  The halving
 *                       after every `rescale`-th layer is part of that layer.  Blocking; not inside a capture.
 *   wrk_v6_frame_read : TensorGpu::back of one frame buffer by name, in its own dtype.  f16: x, att_x, att_xx, aux_x, att_sx (5 planes
 *                       [5][num_token][D]), att_w, att_g, att_o, tmx, tmt, tm (5 planes), ffn_x, ffn_kx, ffn_rx, ffn_k, ffn_v, ffn_r;
 *                       f32: att_k, att_v, att_r, time_decay.  dst NULL: only *bytes is set. */
int32_t wrk_v6_infer_layer(wrk_ctx* ctx, wrk_v6_model* model, wrk_v7_state* state, uint32_t layer, const void* x, const uint32_t* cursors,
                           uint32_t num_token, uint32_t mode);
int32_t wrk_v6_frame_read(wrk_ctx* ctx, wrk_v6_model* model, const char* name, uint32_t num_token, void* dst, size_t capacity, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* WRK_HIP_H */
