// Internal host-side structures behind the opaque handles of include/wrk_hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "wrk_hip.h"
#include "wrk_dev_group.h"
#include "wrk_matjob.h"
#include "wrk_queue_dispatch.h"
#include "wrk_beam_select.h"

struct wrk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // submission stream (ops, programs)
    hipStream_t read_stream = nullptr;  // read-back stream (context.rs:148-162 readback thread)
    hipEvent_t read_event = nullptr;
    std::recursive_mutex mu;
    std::string err;
    // Context::encode (ops.rs:79-143) runs on tokio `spawn_blocking` workers while the runtime task submits cached jobs
    // (runtime/mod.rs:139-167).  So an open capture belongs to the ENCODING THREAD and records on a private stream of
    // its own: the submission stream and the read-back stream are never in capture mode, any number of threads may
    // encode at once, and submissions / reads / uploads from other threads proceed meanwhile.  (Guarded by `mu`.)
    std::map<std::thread::id, hipStream_t> sessions;    // open captures
    std::vector<hipStream_t> capture_pool;              // idle capture streams
    // the stream a wrk_op_* call of THIS thread records on: its open capture, else the submission stream
    hipStream_t op_stream() {
        auto it = sessions.find(std::this_thread::get_id());
        return it == sessions.end() ? stream : it->second;
    }
    bool capturing_here() { return sessions.count(std::this_thread::get_id()) != 0; }
    int num_cu = 256;
    void* staging = nullptr;            // pinned host staging for wrk_buf_write
    size_t staging_bytes = 0;
    // scratch of the prefill GEMM (sub-block input sums of the stacked tokens); grown outside captures, never shrunk, one per context:
    // the programs of a context run on one submission stream, in order
    void* gemm_scratch = nullptr;
    size_t gemm_scratch_cap = 0;
};
int32_t wrk_ctx_reserve_gemm_scratch(wrk_ctx* ctx, size_t bytes);      // WRK_OK also when it cannot grow now (inside a capture): the GEMM then keeps its older kernels

struct wrk_buf {
    wrk_ctx* ctx;
    void* ptr;
    size_t bytes;
    std::atomic<int> refs;
};

struct wrk_matrix {
    wrk_ctx* ctx;
    uint32_t kind, k, m, flags;
    uint8_t* data;          // re-laid-out weight stream (device)
    size_t row_bytes;       // device bytes per row (16-byte aligned)
    size_t stored_bytes;    // algorithmic bytes = GGUF/f16 stored size of the tensor
    uint8_t* aux = nullptr;     // Matrix::Fp4 { q }: the 16 f32 levels (device); side tables live in the row planes
    size_t aux_bytes = 0;
    std::atomic<int> refs;
    float out_scale = 1.0f;     // y = out_scale * (W . x): the 2^-k layer discount of load_matrix_discount kept OUT of the blocks
};

struct wrk_program {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

inline int32_t wrk_fail(wrk_ctx* ctx, int32_t code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int32_t wrk_fail(wrk_ctx* ctx, int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define WRK_HIP(ctx, expr)                                                                              \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return wrk_fail((ctx), _e == hipErrorOutOfMemory ? WRK_E_OOM : WRK_E_HIP, "%s: %s (%s:%d)", \
                            #expr, hipGetErrorString(_e), __FILE__, __LINE__);                          \
    } while (0)

#define WRK_ARG(ctx, cond, ...)                                     \
    do {                                                            \
        if (!(cond)) return wrk_fail((ctx), WRK_E_ARG, __VA_ARGS__); \
    } while (0)

#define WRK_LAUNCH_CHECK(ctx) WRK_HIP(ctx, hipGetLastError())

// ------------------------------------------------------------------ what the blocking row functions share (wrk_api.hip)
inline bool finite_f32(float x) { return std::isfinite(x); }
// The argument checks of a blocking call `who` on n rows of V logits, `stride` floats apart, in `logits`; the caller holds ctx->mu.
// WRK_E_ARG inside a capture of this thread and, with n > 0, unless V >= 1 && stride >= V or when the rows exceed the buffer;
// WRK_E_UNSUPPORTED when max_vocab != 0 and V > max_vocab
int32_t wrk_rows_check(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const char* who, uint32_t max_vocab);
// Temporary device memory of a blocking call, laid out as wrk_dev_layout (wrk_dev_group.h) says: add() every piece first, then alloc()
// once, then at<T>(offset); freed when it goes out of scope
struct wrk_dev_arena : wrk_dev_layout {
    char* base = nullptr;
    wrk_dev_arena() = default;
    wrk_dev_arena(const wrk_dev_arena&) = delete;
    wrk_dev_arena& operator=(const wrk_dev_arena&) = delete;
    ~wrk_dev_arena() { if (base) hipFree(base); }
    hipError_t alloc() { return hipMalloc((void**)&base, total ? total : 256); }
    template <class T> T* at(size_t o) const { return (T*)(base + o); }
};

// ------------------------------------------------------------------ device-side tensor descriptor (DTensor: wrk_matjob.h)
inline DTensor make_dtensor(const wrk_tensor* t) {
    DTensor d;
    d.p = t->buf ? t->buf->ptr : nullptr;
    d.dtype = t->dtype;
    for (int i = 0; i < 4; ++i) {
        d.shape[i] = t->view.shape[i];
        d.stride[i] = t->view.stride[i];
        d.offset[i] = t->view.offset[i];
    }
    return d;
}

inline DTensor make_dense(void* p, uint32_t dtype, uint32_t c, uint32_t t = 1, uint32_t b = 1, uint32_t w = 1) {
    DTensor d;
    d.p = p;
    d.dtype = dtype;
    d.shape[0] = c; d.shape[1] = t; d.shape[2] = b; d.shape[3] = w;
    d.stride[0] = c; d.stride[1] = t; d.stride[2] = b; d.stride[3] = w;
    d.offset[0] = d.offset[1] = d.offset[2] = d.offset[3] = 0;
    return d;
}

inline size_t dtype_size(uint32_t dt) { return dt == WRK_F16 ? 2 : (dt == WRK_U8 ? 1 : 4); }

// number of elements the view's parent tensor must hold for the view to be in bounds
inline size_t dtensor_extent(const DTensor& d) {
    size_t s0 = d.stride[0], s1 = d.stride[1], s2 = d.stride[2] ? d.stride[2] : 1;
    size_t last_w = (size_t)d.offset[3] + (d.shape[3] ? d.shape[3] - 1 : 0);
    size_t last_b = (size_t)d.offset[2] + (d.shape[2] ? d.shape[2] - 1 : 0);
    size_t last_t = (size_t)d.offset[1] + (d.shape[1] ? d.shape[1] - 1 : 0);
    size_t last_c = (size_t)d.offset[0] + (d.shape[0] ? d.shape[0] - 1 : 0);
    return ((last_w * s2 + last_b) * s1 + last_t) * s0 + last_c + 1;
}

// ------------------------------------------------------------------ internal launchers (stream ordered)
namespace wrk {

// wrk_ops.hip
void layer_norm(hipStream_t s, const void* w, const void* b, DTensor x, float eps);
void layer_norm_from(hipStream_t s, const void* w, const void* b, DTensor src, DTensor x, float eps);     // x = LN(src), same shapes
void group_norm(hipStream_t s, const void* w, const void* b, DTensor x, float eps);
void l2_norm(hipStream_t s, DTensor x, float eps);
void token_shift(hipStream_t s, const uint32_t* cursors, DTensor mix, DTensor state, DTensor in, DTensor out, int reversed);
// merged element-wise stages of an RWKV-7 layer over dense f16 [D, T] rows with 64-wide heads (bit-identical to the op chain)
void pre_wkv_v7(hipStream_t s, void* w, void* a, void* k, void* v, void* vv, void* v0, void* n, const void* w0, const void* a0, const void* k_k,
                const void* k_a, const void* v0p, uint32_t D, uint32_t T, bool first_layer, float l2_eps, float* wdec = nullptr);
void post_wkv_v7(hipStream_t s, void* x, const void* r, const void* g, const void* n, const void* gn_w, const void* gn_b, const void* r_k,
                 uint32_t D, uint32_t T, float gn_eps);
// n <= 6 token_shift ops over the same input / state row in one pass (falls back to n launches for views it cannot vectorise)
void token_shift_multi(hipStream_t s, const uint32_t* cursors, const DTensor* mix, const DTensor* out, int n, DTensor state, DTensor in, int reversed);
void transpose(hipStream_t s, DTensor in, DTensor out);
void time_mix_v6(hipStream_t s, const uint32_t* cursors, DTensor decay, const void* u_f32, DTensor state, DTensor k, DTensor v, DTensor r, DTensor x,
                 uint32_t nseq_hint = 0);      // 0: unknown (as many sequences as the state has batches)
void channel_mix_v6(hipStream_t s, const uint32_t* cursors, DTensor state, DTensor r, DTensor v, DTensor x);
void binary(hipStream_t s, int is_mul, DTensor in, DTensor out, uint32_t ax, uint32_t ay, uint32_t ao);
void lerp(hipStream_t s, DTensor x, DTensor y, DTensor f, int reversed);
void blit(hipStream_t s, DTensor in, DTensor out);
void affine(hipStream_t s, DTensor x, float scale, float bias);
void activate(hipStream_t s, DTensor x, uint32_t act);
void control_k_v7(hipStream_t s, const void* p, DTensor a, DTensor k);
void time_mix_v7(hipStream_t s, const uint32_t* cursors, DTensor state, DTensor r, DTensor w, DTensor n, DTensor x, uint32_t nseq_hint = 0, const float* wdec = nullptr);   // nseq_hint 0: unknown; wdec: precomputed decays f32 [D, T] (pre_wkv_v7) or nullptr
void time_first_v7(hipStream_t s, const void* u, DTensor r, DTensor n, DTensor x);
void channel_mix_v7(hipStream_t s, const uint32_t* cursors, DTensor state, DTensor v, DTensor x);
void softmax(hipStream_t s, DTensor x);
void gather_rows_f16(hipStream_t s, const void* table, const uint32_t* ids, void* out, uint32_t d, uint32_t n);
void gather_rows_any(hipStream_t s, DTensor in, const uint32_t* rows, DTensor out, uint32_t n);
void argmax_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t v_stride, uint32_t n, uint32_t* out);

// wrk_sample.hip: examples/chat.rs:150-190 Sampler::sample per row (nucleus cut at top_p, temperature inside it, inverse-CDF draw with
// the SplitMix64 uniform of (seed, *step - step_base)); temperature or top_p == 0 is argmax_rows.  -1: v == 0, v > SAMPLE_MAX_VOCAB or
// stride < v.  step_base is 0 everywhere but in queue programs (wrk_queue.hip), where a request's draws are numbered from its own reply.
// SampleParam and the other rows that a queue dispatch writes (SampleFilter, SampleAlt, PenaltyParam, DryParam): wrk_queue_dispatch.h
static constexpr uint32_t SAMPLE_MAX_VOCAB = 1u << 20;
// One RowGate says whether a row's draw counts: flag == nullptr always, else iff flag[row * stride] == eq (a stop program:
// StopParam::done == 0; a queue program: QueueSlot::phase == QUEUE_REPLY).  The Mirostat sampler moves mu and occurrence_update counts
// the draw under the same gate
struct RowGate { const uint32_t* flag; uint32_t stride, eq; };
// SAMPLE_FILT: two more cuts of the candidates per row, one SampleFilter per row: the first min(n_P, n_K, n_M) ranks
// stay, n_K = top_k (0 or >= v: v; 1: the arg-max, as temperature 0) and n_M = #{fl32(l - max) >= ln_min_p} (-inf: v).  Both off:
// SAMPLE_PLAIN's token, bit for bit
// The two samplers whose candidates are not one of the plain sampler's cuts, one SampleAlt per row next to SampleParam.
// SAMPLE_MIRO: Mirostat v2 -- candidates = rank 0 and every token whose surprise log2 W - (l - max) / T * log2 e is <= mu (top_p is not
// read), then mu <- mu - eta * (s - tau) with s the drawn token's surprise among the candidates; tau == 0: SAMPLE_PLAIN's token, bit for
// bit, mu untouched, and the greedy branch leaves mu alone too.  The update is made iff the row's draw counts (gate).
// SAMPLE_TYP: locally typical sampling -- candidates = the tokens, by |(max - l) - gbar| ascending (ties by index), whose preceding
// softmax mass is <= typical_p (top_p is not read); typical_p >= 1: SAMPLE_PLAIN's token, bit for bit.  alt is only read
// SAMPLE_CUT: SAMPLE_FILT's candidates cut further, one SampleCut per row next to the SampleFilter.  The candidates are
// ranks [m0, n): n = min(n_P, n_K, n_M, n_S, n_E, n_H), each new count a prefix with rank 0 always in -- n_S = #{max - l <= top_n_sigma *
// sigma} (sigma: population deviation of the finite logits), n_E = #{p >= epsilon}, n_H = #{p >= min(eta, sqrt(eta) exp(-H))} -- and XTC:
// with m' = min(#{p >= xtc_threshold}, n) >= 2 and the row's coin below xtc_probability, m0 = m' - 1, else 0.  p is the whole row's
// softmax at temperature 1.  The coin is (SplitMix64's second output of the state that gives u) >> 40, times 2^-24:
// sample_splitmix_next.  All five off: SAMPLE_FILT's token, bit for bit
enum : int { SAMPLE_PLAIN = 0, SAMPLE_FILT = 1, SAMPLE_MIRO = 2, SAMPLE_TYP = 3, SAMPLE_CUT = 4 };
// which sampler, and its rows: par always, filt with SAMPLE_FILT / SAMPLE_CUT, alt with SAMPLE_MIRO / SAMPLE_TYP, gate with SAMPLE_MIRO,
// cut with SAMPLE_CUT
struct SamplePick { int mode; const SampleParam* par; const SampleFilter* filt; SampleAlt* alt; RowGate gate; const SampleCut* cut = nullptr; };
int sample_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const SamplePick& pick, const uint32_t* step,
                uint32_t* out);

// wrk_score.hip: per row, logprob = x_t - logsumexp(x) and rank = #{x_i > x_t} + #{i < t : x_i == x_t} of the target t = targets[row]
// (targets < v: the caller validates them).  Each row is split over score_slices(n, v, num_cu) workgroups; part holds n * that many
// partials (at most n * SCORE_MAX_SLICES).  -1: v == 0 or stride < v
struct ScorePart { float m, s; uint32_t gt, eq; };
static constexpr uint32_t SCORE_MAX_SLICES = 32;
uint32_t score_slices(uint32_t n, uint32_t v, int num_cu);
int score_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* targets, ScorePart* part,
               float* logprob, uint32_t* rank, int num_cu);

// wrk_logprob.hip: per row, the log-prob of the chosen token tokens[row] (< v, else NaN) and the num_top first tokens of the sampler's
// order with their log-probs, on the raw logits.  LogprobParam is device data, in a decode loop a per-frame block written
// before every call: the output buffers and num_top (<= LOGPROB_MAX_TOP), so one captured program serves any num_top.  Row r goes to row
// (step ? *step : 0) * n + r of logprob [cap_rows], top_ids / top_logprobs [cap_rows][num_top]; a row at or past cap_rows is not written.
// part / keys: scratch of logprob_part_bytes(n) / logprob_key_bytes(n).  -1: v == 0, v > SAMPLE_MAX_VOCAB or stride < v
static constexpr uint32_t LOGPROB_MAX_TOP = WRK_MAX_TOP_LOGPROBS;
struct LogprobParam { float* logprob; uint32_t* top_ids; float* top_logprobs; uint32_t num_top, cap_rows; };
struct LogprobPart { float m, s; };
inline size_t logprob_part_bytes(uint32_t n) { return (size_t)n * SCORE_MAX_SLICES * sizeof(LogprobPart); }
inline size_t logprob_key_bytes(uint32_t n) { return (size_t)n * SCORE_MAX_SLICES * 4 * LOGPROB_MAX_TOP * 8; }
int logprob_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const uint32_t* tokens, const uint32_t* step,
                 const LogprobParam* par, LogprobPart* part, unsigned long long* keys, int num_cu);

// wrk_penalty.hip: repetition penalties.  One PenaltyParam per row: the row's slot of an occurrence table (count f32 [v],
// flags u8 [v]: bit 0 present, bit 1 banned), the table's weights f32 [v] and the sequence's (presence, frequency, decay).  Decode loops
// keep these in a per-frame device buffer written before every call, so a captured step never holds a table pointer of its own.
// penalize_rows: dst row r = the penalised src row r (src == dst allowed).  occurrence_update: row r applies tokens[r * ntok ..] in
// order (count *= decay, then count[y] += weight[y], present[y] = 1); tokens < v (the caller validates them).  A row whose draw does not
// count (gate: a finished sequence of a stop program, a prompt-phase or idle slot of a queue program) is left alone
void penalize_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, const PenaltyParam* par, float* dst,
                   uint32_t dst_stride);
void occurrence_update(hipStream_t s, uint32_t v, uint32_t n, const PenaltyParam* par, const uint32_t* tokens, uint32_t ntok, const RowGate& gate);

// wrk_grammar.hip: constrained decoding.  A grammar is a DFA over token ids with alphabet compression: token_class u16 [v]
// and transitions u16 [states][num_classes], WRK_GRAMMAR_REJECT for a class that is not allowed.  GrammarParam is device data, in a
// decode loop a per-frame block written before every call: the two tables, num_classes and the per-row state words, so a captured step
// never holds a table pointer of its own.  constrain_rows: dst row r = src row r with the bits of -inf wherever the token is not allowed
// in states[r], the source bits elsewhere (src == dst allowed).  grammar_advance: states[r] <- the next state on tokens[r]; a rejected
// token, and a row whose draw does not count (gate), leave it alone
struct GrammarParam { const uint16_t* token_class; const uint16_t* transitions; uint32_t num_classes, pad; uint32_t* states; };
void constrain_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, const GrammarParam* par, float* dst,
                    uint32_t dst_stride);
void grammar_advance(hipStream_t s, uint32_t v, uint32_t n, const GrammarParam* par, const uint32_t* tokens, const RowGate& gate);

// wrk_bias.hip: logit bias.  A wrk_logit_bias is one CSR of bias sets, every set sorted by id: set s is the pairs
// (ids[e], values[e]), e in [offsets[s], offsets[s + 1]).  BiasParam is device data, in a decode loop a per-frame block written before
// every call: the object's three arrays and the per-row set words (WRK_BIAS_NONE: the row is left alone), so a captured step never holds
// a pointer of the object.  bias_rows: out row r = in row r with -inf (its bits) at every id of the row's set whose value is -inf,
// in + value at every other id of the set, the source bits elsewhere; in == out (same stride): in place, only the entries are applied
struct BiasParam { const uint32_t* offsets; const uint32_t* ids; const float* values; const uint32_t* sets; };
void bias_rows(hipStream_t s, const float* in, uint32_t v, uint32_t in_stride, uint32_t n, const BiasParam* par, float* out, uint32_t out_stride);

// wrk_guide.hip: classifier-free guidance.  guide_rows: out row r = the guided row of in rows r (conditional) and n + r
// (unconditional) with the scale par[r], device data, in a decode loop a per-frame buffer written before every call; a row with scale 1
// is the conditional row bit for bit.  guide_follow: argmax[n + r] = argmax[r], the partner sequences take the conditional ones' draws
void guide_rows(hipStream_t s, const float* in, uint32_t v, uint32_t in_stride, uint32_t n, const float* par, float* out, uint32_t out_stride);
void guide_follow(hipStream_t s, uint32_t* argmax, uint32_t n);

// wrk_dry.hip: DRY and the no-repeat-n-gram ban.  One DryParam per row: the row's slot of a token window -- ring [cap] of
// ids, meta = (length, next write position) -- and the row's values, pen[m] the host-computed penalty of a match of m tokens (0 below
// allowed_length).  DryBreakers: the call's breaker ids.  Both are device data, in a decode loop per-frame buffers written before
// every call, so a captured step never holds a window pointer of its own.  dry_rows: row r of x [n][stride] in place -- per token the
// longest match M that the token would extend (text-generation-webui's loop, capped at WRK_DRY_MAX_MATCH), then -inf for
// no_repeat != 0 && M >= no_repeat - 1, else x - pen[M] for multiplier != 0 && M >= allowed; every other element keeps its bits.
// scratch: u32 [n][v], all zero before and after every launch.  copy_rows: dst row r = src row r, bit for bit (the head output into the
// rows dry_rows then works on).  window_push: slot r takes tokens[r]; a row whose draw does not count (gate) is left alone
struct DryBreakers { uint32_t count; uint32_t ids[WRK_MAX_DRY_BREAKERS]; };
void dry_rows(hipStream_t s, float* x, uint32_t v, uint32_t stride, uint32_t n, const DryParam* par, const DryBreakers* brk, uint32_t* scratch);
void copy_rows(hipStream_t s, const float* src, uint32_t v, uint32_t src_stride, uint32_t n, float* dst, uint32_t dst_stride);
void window_push(hipStream_t s, uint32_t v, uint32_t n, const DryParam* par, const uint32_t* tokens, const RowGate& gate);

// wrk_stop.hip: stop tokens in the decode loops.  One StopParam per sequence in a per-frame device buffer written
// before every call: the stop ids are data, one captured program serves any stop sets.  done / length / end_token are the device's:
// the step that draws a stop id sets them (length = step + 1: the stop token is part of the output)
struct StopParam { uint32_t ids[WRK_MAX_STOP_TOKENS]; uint32_t count, done, length, end_token; };
// a frame's stop buffers and the state they snapshot: sequences [b0, b0 + B) of a state [L][num_batch][slot] f32
struct StopGeom {
    float *state, *head_o, *snap_state, *snap_logits;
    const uint32_t* just_ended; const StopParam* par; const uint32_t* counter; uint32_t* lengths;
    uint32_t layers, num_batch, b0, v;
    size_t slot;
};
// tokens / history <- drawn (or the ending token of a finished sequence), stop check, just_ended[b], *live -= sequences that ended,
// counter += 1 last (the sampler reads it)
void advance_stop(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, StopParam* par,
                  uint32_t* just_ended, uint32_t* live, uint32_t b);
// state slot and head_o row of every sequence with just_ended[b] -> snapshot (workgroups of the others return at once)
void stop_snapshot(hipStream_t s, const StopGeom& g, uint32_t b, int num_cu);
// snapshot -> state slot and head_o row of every sequence that is done; lengths[b] = its length, or *counter if it never ended
void stop_restore(hipStream_t s, const StopGeom& g, uint32_t b, int num_cu);

// Stop sequences (the matcher itself: wrk_stopseq_dev.h).  StopSeqRow: one owner's stop sequences as device data, each
// stored REVERSED (tok[k][0] is sequence k's last id), so that the usual step rejects a sequence after one compare with the drawn token.
// An owner's tail is WRK_STOP_TAIL_LEN words, oldest first, right aligned, WRK_STOP_TAIL_EMPTY for a missing entry -- the ABI's layout
struct StopSeqRow { uint32_t count, pad[3]; uint32_t len[WRK_MAX_STOP_SEQUENCES]; uint32_t tok[WRK_MAX_STOP_SEQUENCES][WRK_MAX_STOP_SEQUENCE_LEN]; };
// the stop-sequence buffers of a stop program: rows [B], tails [B][WRK_STOP_TAIL_LEN], match words [B] (NONE until the sequence ends)
struct StopSeqBufs { const StopSeqRow* rows; uint32_t* tail; uint32_t* match; };
// advance_stop for stop programs with sequences: the same ownership and ordering; a sequence ends on its stop set or on a stop
// sequence, and the step also writes its tail and, where it ends, its match word
void advance_stop_seq(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, StopParam* par,
                      uint32_t* just_ended, uint32_t* live, const StopSeqBufs& q, uint32_t b);
// one counted draw of n owners (wrk_stop_sequences_advance): row r's stop sequences rows[r], its stop set ids[r] (nullptr: none; only
// ids / count of a StopParam are read), tail[r] in / out, tokens[r], match[r] out
void stop_seq_rows(hipStream_t s, uint32_t n, const StopSeqRow* rows, const StopParam* ids, uint32_t* tail, const uint32_t* tokens, uint32_t* match);

// wrk_queue.hip: a request queue in the decode loops.  Its structures (QueueReq ... QueueBufs, QueueStateBufs) and its
// dispatch rule: wrk_queue_dispatch.h.
// advance_queue takes advance_tokens' place in a queue program: history <- drawn; per slot the next prompt token or the draw, stop / max_new check,
// next requests to the slots that ended (ascending slot order), their parameters into the slot's rows, started[b], the log,
// ctl->live -= ended, counter += 1 last (the sampler reads it)
void advance_queue(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q, uint32_t b);
// slots [b0, b0 + b) of a state [L][num_batch][slot] f32 with started[b]: zero fill, or a copy of ctl->init_state; with pen_par their
// occurrence rows: count = 0, present bit cleared, banned bit kept (v: vocabulary).  Workgroups of the other slots return at once
struct QueueGeom { float* state; uint32_t layers, num_batch, b0, v; size_t slot; };
void queue_reset(hipStream_t s, const QueueGeom& g, const QueueBufs& q, uint32_t b, int num_cu);
// A guided queue (the rule: queue_dispatch_guided): `pairs` request slots, pair i = slots i and pairs + i of q.slots /
// q.started / tokens / drawn (guide_follow has copied the draw of row i to row pairs + i) and of the state; pairs <= 128; q has the four
// guided arrays and pair_started.  advance_queue_guided: advance_queue over the pairs, the history 2 * pairs wide.  queue_reset_guided:
// queue_reset over the 2 * pairs state slots by q.started, a partner slot from ctl->negative_init_state, and the occurrence rows of the
// pairs by q.pair_started
void advance_queue_guided(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q,
                          uint32_t pairs);
void queue_reset_guided(hipStream_t s, const QueueGeom& g, const QueueBufs& q, uint32_t pairs, int num_cu);
// A state pool under the queue: P states in wrk_v7_state_read's layout in one device buffer; request r may start from a
// copy of entry start[r] and has its end state written to entry save[r] in the step that ends it.  QueueStateCtl: the pool's pointer and
// entry count are data (one captured program serves any pool), next to the length of the step's turnover list (QueueTurn).
// QueueHistory: a history pool beside the state pool, entry k of it belonging to entry k of the states: count f32
// [entries][v] and flags u8 [entries][v] (the present bit only), and with cap > 0 ring u32 [entries][cap] and meta u32 [entries][2]
// (length, next write position) -- what an occurrence slot and a token-window slot hold.  All nullptr / 0: none.  Device data as the
// states' pointer is: one captured program serves any history pool
struct QueueHistory { float* count; uint8_t* flags; uint32_t* ring; uint32_t* meta; uint32_t cap, pad; };
struct QueueStateCtl { float* states; uint32_t num_entries, turn_count; QueueHistory hist; };
// advance_queue for pool programs: the same body, and the step's turnover list
void advance_queue_pool(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q,
                        const QueueStateBufs& p, uint32_t b);
// queue_reset for pool programs: a (layers x slices) grid that does not grow with b loops over the turnover list -- per 16-byte element
// load the slot, store it to the save entry, then store the start entry / init_state / zero to the slot, in one thread -- and the
// occurrence rows as queue_reset.  g.slot % 4 == 0 and 16-byte aligned bases only (the callers check)
void queue_turnover(hipStream_t s, const QueueGeom& g, const QueueBufs& q, const QueueStateBufs& p, uint32_t b, int num_cu);
// The turnover of the slots' contexts in a call with a history pool, and the copy kernel of wrk_history_pool_put / _get: one grid of
// ceil(v / 1024) + ceil(WRK_MAX_TOKEN_WINDOW / 1024) workgroups, whatever b and whatever the windows' capacity, walks the turnover list.  Per element of a listed slot, in one thread: load
// the slot (pen[slot]'s count / flags, dry[slot]'s ring / meta), store it to the save entry (the present bit only), then store the
// slot's new value -- the start entry's, or count 0 / no present bit / an empty window -- keeping the slot's banned bits.  pen or dry
// may be nullptr (no occurrence rows / no windows in the call); 16-byte elements when v % 4 == 0, scalar otherwise
void queue_history_turnover(hipStream_t s, uint32_t v, const QueueStateCtl* sctl, const QueueTurn* turn, const PenaltyParam* pen,
                            const DryParam* dry);

// wrk_beam.hip: beam search in the decode loops (the rule itself: wrk_beam_select.h).  BeamParam is device data, in a
// decode loop a per-frame block written before every call: W, the number of groups and how many history rows and inv_norm entries
// there are, so one captured program serves any W.  BeamBufs: the slot records [B], the groups' stop sets, the host's inv_norm table,
// the candidate front's output (ids / lp [B][W]: wrk_top_logprobs' top arrays of the rows with num_top = W), the step history
// [hist_rows][B] x 3, the step's copy list copy_src [B] (NO_COPY: the slot moves no bytes), snap_map [B] (q where slot q ended in this
// step, else NO_COPY), done_map [B] (q where slot q is DONE, else NO_COPY), the count of LIVE slots and filled [B] (1 where the step
// gave slot q a token, LIVE or DONE, else 0: the gate of a beam context's updates, written for every slot in every step)
struct BeamParam { uint32_t w, groups, hist_rows, inv_len; };
struct BeamBufs {
    const BeamParam* par; BeamSlot* slots; const BeamStop* stops; const float* inv_norm;
    const uint32_t* cand_ids; const float* cand_lp;
    uint32_t *step_tokens, *step_parents; float* step_scores;
    uint32_t *copy_src, *snap_map, *done_map, *live, *filled;
};
// the candidate front and the selection of one step over rows [b][stride] (v used): logprob_rows with `lp` (num_top = W, its top arrays
// Q.cand_ids / Q.cand_lp) on the chosen tokens lp_tokens (any ids < v), then beam_select: one workgroup, a wave per group; writes the
// records, tokens[q] of every slot filled, row *counter of the history, the three maps, *live, and moves the counter last.
// -1: logprob_rows' refusals
int beam_step_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t b, const uint32_t* lp_tokens, const LogprobParam* lp,
                   LogprobPart* part, unsigned long long* keys, const BeamBufs& Q, uint32_t* tokens, uint32_t* counter, int num_cu);
// Slot copies over all layers between two arrays of slots, layer l's slot i of an array at base + ((size_t)l * nb + b0 + i) * slot:
// for every q < n with map[q] != WRK_BEAM_NO_COPY, dst slot q <- src slot (src_mapped ? map[q] : q).  16-byte copies cut over about two
// workgroups per CU (scalar ones unless slot % 4 == 0 and both bases are 16-byte aligned); workgroups of the other slots return at
// once.  src and dst do not overlap
struct BeamSlots { float* base; uint32_t nb, b0; };
void beam_copy(hipStream_t s, const BeamSlots& src, const BeamSlots& dst, uint32_t layers, size_t slot, const uint32_t* map, bool src_mapped,
               uint32_t n, int num_cu);
// state slot q <- state slot map[q] for the listed q, under any aliasing: a gather into `scratch` (n slots per layer), then the scatter
void beam_permute(hipStream_t s, const BeamSlots& state, float* scratch, uint32_t layers, size_t slot, const uint32_t* map, uint32_t n, int num_cu);
// A beam context: what a hypothesis carries beside its state -- its occurrence row (counts and both flag bits), its token
// window (ring and the two meta words) and its automaton state -- found through the rows' own parameter blocks: pen[q] / dry[q] name slot
// q's row and window (nullptr: the call has none), gram the state words [n] (nullptr: none).  BeamCtxScratch: n context rows, counts
// [n][v], flags [n][v], rings [n][the window's capacity], meta [n][2], states [n].
// beam_context_permute: slot q's context <- slot map[q]'s for every q < n with map[q] != WRK_BEAM_NO_COPY, under any aliasing: a gather
// into the scratch, then the scatter, as beam_permute.  The grid is ceil(max(v, WRK_MAX_TOKEN_WINDOW) / 1024) x n whatever the map and
// the capacity, which is data; workgroups of unlisted slots return at once.  16-byte moves of the counts (4-byte ones of the flags) when
// v % 4 == 0 and of a ring when its capacity % 4 == 0, scalar moves otherwise
struct BeamCtxRows { const PenaltyParam* pen; const DryParam* dry; uint32_t* gram; };
struct BeamCtxScratch { float* count; uint8_t* flags; uint32_t* ring; uint32_t* meta; uint32_t* gram; };
void beam_context_permute(hipStream_t s, const BeamCtxRows& rows, const BeamCtxScratch& scratch, uint32_t v, const uint32_t* map, uint32_t n);

// WRK_TIMING=1 (debug): in-kernel wall-clock stamps of one decode layer, printed after wrk_v7_generate_greedy
unsigned long long* timing_slot(wrk_ctx* ctx, const char* label);   // nullptr unless enabled
void timing_report(wrk_ctx* ctx);

// wrk_matvec.hip (MatJob: wrk_matjob.h)
uint32_t matvec_num_wg(const MatJob* jobs, int njobs, int num_cu, uint32_t* rows_per_wg);
// dry_run: classify only (0 = a launch would honour every job's prologue / carry request, -3 = it cannot)
// dmv_only: with 2 .. 4 input vectors, -5 unless the multi-token dmv kernels take the launch (the caller then prefers the matrix cores)
int matvec(hipStream_t s, const MatJob* jobs, int njobs, int num_cu, bool dry_run = false, bool no_catchall = false, bool dmv_only = false);
// as matvec, but jobs of several quantised kinds are split into one launch per kind (F16 jobs ride with the first)
int matvec_grouped(hipStream_t s, const MatJob* jobs, int njobs, int num_cu, bool dry_run = false);
// MFMA dequant-GEMM (wrk_gemm.hip); -2 = not applicable (caller uses the matvec kernels)
int matmul_mfma(hipStream_t s, const MatJob& job, int num_cu);
// several matrices x the same tokens in ONE launch (-2 if any job is not for the MFMA path)
int matmul_mfma_multi(hipStream_t s, const MatJob* jobs, int njobs, int num_cu);
// The chain every matmul call site runs: the jobs as one MFMA group, else per matrix on the MFMA path, else per matrix on the matvec
// kernels.  With `tokens` (the caller's step; a head launch may have fewer rows of its own) below gemm_min_tokens() the matvec kernels at
// once, per matrix or as one matvec_grouped call (few).  ks: scratch of the K-sliced GEMM, t3: of the third-generation prefill tile; both
// go to job 0 only (a launch reads them from its first job), nullptr = none: that kernel is not used.  Returns 0 or the failing launch's
// code, with *bad (if given) the job it was for
struct KsScratch { float* part; uint32_t* cnt; size_t part_cap; uint32_t cnt_cap; };
struct T3Scratch { void* p; size_t cap; };
enum class FewTokens { matvec_each, matvec_grouped };
int matmul_jobs(hipStream_t s, MatJob* jobs, int n, uint32_t tokens, int num_cu, const KsScratch* ks, const T3Scratch* t3, FewTokens few, int* bad = nullptr);
uint32_t gemm_min_tokens();
// wrk_quant.hip
void quantize_int8(hipStream_t s, const void* src_f16, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes);
void quantize_nf4(hipStream_t s, const void* src_f16, const float* levels, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes);
size_t repack_row_bytes(uint32_t kind, uint32_t k);
uint32_t int8_row_blocks(uint32_t k);   // (min, max) entries stored per Int8 row
int repack_rows(uint32_t kind, uint32_t k, uint32_t m, const uint8_t* src, uint8_t* dst);   // host side
size_t stored_bytes(uint32_t kind, uint32_t k, uint32_t m);

}  // namespace wrk

// validated per-sequence sampler parameters (WRK_E_ARG on NULL arrays or a NaN / negative temperature or top_p)
int32_t wrk_sample_pack(wrk_ctx* ctx, const float* temperature, const float* top_p, const uint32_t* seed, uint32_t n,
                        std::vector<wrk::SampleParam>& out);
// validated per-sequence filter rows; either array may be NULL (off).  WRK_E_ARG on a min_p that is NaN or outside [0, 1]
int32_t wrk_filter_pack(wrk_ctx* ctx, const uint32_t* top_k, const float* min_p, uint32_t n, std::vector<wrk::SampleFilter>& out);
// the cut sampler's per-sequence arrays, any of which may be NULL (off), validated into rows.  WRK_E_ARG on a NaN or
// negative value, on an epsilon_cutoff, eta_cutoff, xtc_probability or xtc_threshold outside [0, 1] and on one of the two XTC arrays alone
struct wrk_cut_args {
    const float *top_n_sigma = nullptr, *epsilon_cutoff = nullptr, *eta_cutoff = nullptr, *xtc_probability = nullptr, *xtc_threshold = nullptr;
    bool any() const { return top_n_sigma || epsilon_cutoff || eta_cutoff || xtc_probability || xtc_threshold; }
};
int32_t wrk_cut_pack(wrk_ctx* ctx, const wrk_cut_args& a, uint32_t n, std::vector<wrk::SampleCut>& out);
// validated per-sequence SampleAlt rows of a Mirostat call (tau required; eta NULL: 0; mu NULL: 2 tau) or of a typical call (typical_p).
// WRK_E_ARG on NaN, negative or non-finite tau / eta, a non-finite mu, a typical_p that is NaN or outside [0, 1]
int32_t wrk_mirostat_pack(wrk_ctx* ctx, const float* tau, const float* eta, const float* mu, uint32_t n, std::vector<wrk::SampleAlt>& out);
int32_t wrk_typical_pack(wrk_ctx* ctx, const float* typical_p, uint32_t n, std::vector<wrk::SampleAlt>& out);

// WRK_E_ARG unless every target < V (targets may be NULL only when n == 0)
int32_t wrk_score_check_targets(wrk_ctx* ctx, const uint32_t* targets, uint32_t n, uint32_t V);

// include/wrk_hip.h wrk_occurrence: one allocation holding counts f32 [num_batch][num_vocab], weights f32 [num_vocab] and
// flags u8 [num_batch][num_vocab] (bit 0 present, bit 1 banned)
struct wrk_occurrence {
    wrk_ctx* ctx = nullptr;
    uint32_t num_batch = 0, num_vocab = 0;
    void* mem = nullptr;
    float* counts = nullptr;
    float* weights = nullptr;
    uint8_t* flags = nullptr;
    wrk::PenaltyParam row(uint32_t slot, float presence, float frequency, float decay) const;
};
// validated PenaltyParam rows of slots [first, first + n) (WRK_E_ARG on a NULL table or array, a table of another context or another
// vocabulary, slots out of range, a non-finite presence / frequency, a decay outside [0, 1]); decay NULL: 1
int32_t wrk_penalty_pack(wrk_ctx* ctx, const wrk_occurrence* occ, uint32_t first, uint32_t n, uint32_t V, const float* presence,
                         const float* frequency, const float* decay, std::vector<wrk::PenaltyParam>& out);

// include/wrk_hip.h wrk_grammar: one allocation holding token_class u16 [num_vocab] and transitions u16 [num_states][num_classes]
struct wrk_grammar {
    wrk_ctx* ctx = nullptr;
    uint32_t num_vocab = 0, num_states = 0, num_classes = 0;
    void* mem = nullptr;
    uint16_t* token_class = nullptr;
    uint16_t* transitions = nullptr;
    wrk::GrammarParam param(uint32_t* states) const;
};
// validated start states of n rows (WRK_E_ARG on a NULL grammar, a grammar of another context or another vocabulary, a state >=
// num_states); state NULL: all 0
int32_t wrk_grammar_pack(wrk_ctx* ctx, const wrk_grammar* g, const uint32_t* state, uint32_t n, uint32_t V, std::vector<uint32_t>& out);

// include/wrk_hip.h wrk_logit_bias: one allocation holding offsets u32 [num_sets + 1], ids u32 [num_entries] and values f32
// [num_entries], every set sorted by id
struct wrk_logit_bias {
    wrk_ctx* ctx = nullptr;
    uint32_t num_vocab = 0, num_sets = 0, num_entries = 0;
    void* mem = nullptr;
    uint32_t* offsets = nullptr;
    uint32_t* ids = nullptr;
    float* values = nullptr;
    wrk::BiasParam param(const uint32_t* sets) const;
};
// validated set words of n rows (WRK_E_ARG on a NULL object, an object of another context or another vocabulary, a word that is neither
// < num_sets nor WRK_BIAS_NONE); set NULL: all 0
int32_t wrk_bias_pack(wrk_ctx* ctx, const wrk_logit_bias* lb, const uint32_t* set, uint32_t n, uint32_t V, std::vector<uint32_t>& out);

// classifier-free guidance (wrk_guide.hip): validated scales of n rows (WRK_E_ARG on a NULL array with n > 0 and on a scale that is NaN,
// infinite or negative; WRK_E_UNSUPPORTED on a vocabulary above the sampler's limit)
int32_t wrk_guide_pack(wrk_ctx* ctx, const float* scale, uint32_t n, uint32_t V, std::vector<float>& out);

// beam search (wrk_beam.hip): inv_norm[l] = (float)(1.0 / pow((double)l, (double)length_penalty)) for l in [1, max_len], entry 0 unused
// (WRK_E_ARG on a penalty that is negative, infinite or NaN, or whose table leaves the normal numbers); the groups' stop sets from a CSR
// of G + 1 offsets, every set sorted (both arrays NULL: all empty; WRK_E_ARG as wrk_generate_options' stop sets, the cap being
// WRK_MAX_BEAM_STOP_TOKENS)
int32_t wrk_beam_inv_norm(wrk_ctx* ctx, float length_penalty, uint32_t max_len, std::vector<float>& out);
int32_t wrk_beam_stops(wrk_ctx* ctx, const uint32_t* tokens, const uint32_t* off, uint32_t G, uint32_t V, std::vector<wrk::BeamStop>& rows);

// include/wrk_hip.h wrk_token_window: one allocation holding the rings u32 [num_batch][capacity] and meta u32 [num_batch][2]
// (length, next write position)
struct wrk_token_window {
    wrk_ctx* ctx = nullptr;
    uint32_t num_batch = 0, num_vocab = 0, capacity = 0;
    void* mem = nullptr;
    uint32_t* ring = nullptr;
    uint32_t* meta = nullptr;
};
// include/wrk_hip.h wrk_history_pool: one allocation holding counts f32 [num_entries][num_vocab], flags u8 [num_entries][num_vocab]
// (bit 0 present; bit 1 is never set) and, with capacity > 0, rings u32 [num_entries][capacity] and meta u32 [num_entries][2]
struct wrk_history_pool {
    wrk_ctx* ctx = nullptr;
    uint32_t num_entries = 0, num_vocab = 0, capacity = 0;
    void* mem = nullptr;
    float* counts = nullptr;
    uint8_t* flags = nullptr;
    uint32_t* ring = nullptr;
    uint32_t* meta = nullptr;
    wrk::QueueHistory dev() const { return wrk::QueueHistory{counts, flags, ring, meta, capacity, 0u}; }
};
// the DRY fields of a call (wrk_generate_options / wrk_queue_options / wrk_dry_logits); the four parameter arrays may be NULL
struct wrk_dry_args {
    wrk_token_window* window = nullptr;
    const float *multiplier = nullptr, *base = nullptr;
    const uint32_t *allowed_length = nullptr, *no_repeat_ngram = nullptr, *breakers = nullptr;
    uint32_t num_breakers = 0;
    bool any_array() const { return multiplier || base || allowed_length || no_repeat_ngram || breakers || num_breakers; }
};
// validated DryParam rows of n owners and the breaker block (WRK_E_ARG on a NULL window, a window of another context or another
// vocabulary, slots out of range, a value outside its range, too many breakers or one >= V; WRK_E_UNSUPPORTED on V > 2^20).  Row r
// names slot first + r for r < slots, slot `first` beyond (a queue keeps only the values of its request rows)
int32_t wrk_dry_pack(wrk_ctx* ctx, const wrk_dry_args& a, uint32_t first, uint32_t n, uint32_t slots, uint32_t V, std::vector<wrk::DryParam>& rows,
                     wrk::DryBreakers& brk);
