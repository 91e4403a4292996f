// Host-side driver shared by the RWKV-7 and RWKV-6 runners (wrk_v7.hip, wrk_v6.hip): matmul launches, job validation, the
// frame state both models carry, cached step programs, job upload / read-back and the decode loops (wrk_generate,
// wrk_generate_queue).  A runner keeps what is its own -- the scratch layout, enqueue_ops / enqueue_fused_decode, its graph-key
// bits, its lanes -- behind the few virtual methods of wrk_frame_common.
#pragma once
#include <atomic>
#include <functional>
#include <initializer_list>
#include <map>
#include <tuple>
#include <vector>

#include "wrk_internal.h"
#include "wrk_device.h"

struct wrk_v7_state {       // recurrent state of either model family
    // captured graphs bake the state's addresses and strides in: they are keyed by this id, never reused, rather than by
    // the handle's address (a destroyed state's address can come back with another num_batch)
    const void* uid = next_uid();
    static const void* next_uid() { static std::atomic<uintptr_t> n{1}; return (const void*)(n.fetch_add(1) << 4); }
    wrk_ctx* ctx = nullptr;
    uint32_t num_layer = 0, num_emb = 0, head_size = 0, num_batch = 0;
    float* data = nullptr;      // [L][B][S+2][D] f32 == L tensors [D, S+2, B] (v7.rs:514-527)
    size_t layer_elems() const { return (size_t)num_batch * (head_size + 2) * num_emb; }
    float* layer_ptr(uint32_t l) const { return data + layer_elems() * l; }
};

namespace wrk {
// the part of a frame that jobs and decode steps go through, laid out by each model's ensure_scratch (base of V7Scratch / V6Scratch)
struct FrameIo {
    float* head_o;      // f32 logits [V, num_header]
    uint32_t *cursors, *tokens, *headers, *argmax, *counter;
};

MatJob mat_job(const wrk_matrix* m, DTensor in, DTensor out, uint32_t act);

// tokens <- argmax; history[counter][b] = argmax[b]; counter += 1   (one tiny kernel)
void advance_tokens(hipStream_t s, const uint32_t* argmax, uint32_t* tokens, uint32_t* history, uint32_t* counter, uint32_t b);
void argmax_finish(hipStream_t s, const float* pv, const uint32_t* pi, uint32_t nwg, uint32_t ntok, uint32_t* argmax, uint32_t* tokens,
                   uint32_t* history, uint32_t* counter);

// K0 / K4 of the fused decode paths (wrk_v7_fused.hip): layer norm + token shifts of stacked tokens, one workgroup per token
struct LnMixParams {
    const f16* src;             // [T][D] rows, or the embedding table when `ids` is set
    const uint32_t* ids;        // optional row index per token (embedding gather / header rows)
    const f16 *ln_w, *ln_b;
    float eps;
    uint32_t d, nmix;
    const f16* mix[6];          // token-shift factors
    f16* out[6];                // shifted outputs [T][D]
    f16* ln_out;                // optional: LN output [T][D]
    float* state_row;           // optional: shift state row, element (batch, c) at state_row[batch * state_stride + c]
    size_t state_stride;
    const uint32_t* cursors;    // batch id per token
    uint32_t batch1;            // host-known batches: token t is batch batch1 - 1 + t (0: read the cursor)
    uint32_t no_carry;          // 1: leave the shift state alone (a later kernel of the layer still reads it: RWKV-6)
};
int ln_mix(hipStream_t s, const LnMixParams& P, uint32_t T);      // -1: unsupported shape (D % 8, D > 8192, nmix not in {0, 1, 2, 6})
}  // namespace wrk

int32_t wrk_buf_write_raw(wrk_ctx* ctx, void* dst, const void* src, size_t bytes);

// one matrix, or several matrices x the same token count in one MFMA launch per kernel family; per-matrix launches (MFMA GEMM, else
// the matvec kernels) when the grouped GEMM declines
int32_t wrk_mm(wrk_ctx* ctx, const wrk_matrix* m, DTensor in, DTensor out, uint32_t act);
int32_t wrk_mm_group(wrk_ctx* ctx, wrk::MatJob* jobs, int n);

// ------------------------------------------------------------------ one RnnJob (wrk_v*_infer, with `score` wrk_v*_score)
struct wrk_job_args {
    const uint32_t* tokens; const uint16_t* emb_rows;       // token ids, or gathered embedding rows
    const uint32_t* cursors; uint32_t T;
    const uint32_t* headers; uint32_t NH;
    float* logits; uint32_t* argmax;                        // read back when set
    bool score; const uint32_t* targets; float* logprob; uint32_t* rank;
};
struct wrk_job_shape { uint32_t nseq; bool one_token_each, contiguous, identity; };
// validates cursors (batch | token << 8 | len << 24: ranges, one writer per state slice), token ids and header rows on the host -- a bad
// index would fault the GPU -- and derives the job's shape.  contiguous: token t is batch (batch of token 0) + t
int32_t wrk_job_check(wrk_ctx* ctx, const wrk_v7_state* st, const uint32_t* cursors, uint32_t T, const uint32_t* tokens_or_null, uint32_t V,
                      const uint32_t* headers, uint32_t NH, wrk_job_shape* shape);
int32_t wrk_score_check(wrk_ctx* ctx, const wrk_job_args& a, uint32_t V, const char* who);

// What a step program of the decode loops is: how each sequence's next token is picked from head_o, and what follows the pick.
// A filtered pick is a sampled one and a pool tail is a queue tail by construction; wrk_pick_pack sets `penalized` only with a sampled pick
struct wrk_step_kind {
    // arg-max / the sampler (wrk_sample.hip) on sample_par / the filtered sampler, also on filter_par / the Mirostat v2 sampler, also on
    // alt_par, whose mu it carries from draw to draw / the typical sampler, also on alt_par / the cut sampler, on filter_par
    // and cut_par
    enum Pick : uint32_t { GREEDY, SAMPLED, FILTERED, MIROSTAT, TYPICAL, CUT };
    // advance_tokens / wrk_stop.hip / wrk_queue.hip / the same with a state pool / beam search (wrk_beam.hip): no pick at all --
    // on head_o, or biased on bias.out, the candidate front and beam_select, then the slot permutation and the snapshot of the slots that ended
    enum Tail : uint32_t { PLAIN, STOP, QUEUE, QUEUE_POOL, BEAM };
    Pick pick = GREEDY;
    bool penalized = false;     // the pick is made on pen_o = head_o penalised with the occurrence rows of pen_par, which then count the draw (wrk_penalty.hip)
    Tail tail = PLAIN;
    bool logprobs = false;      // between the pick and the tail, the log-prob launches (wrk_logprob.hip) on head_o and the picked tokens, on lp_par
    // the pick is made on the row masked by the automaton of gram_par (wrk_grammar.hip): pen_o masked in place when penalised, else con_o =
    // the masked head_o; the tail then advances the automaton states where it updates the occurrence rows, under the same gate
    bool constrained = false;
    // a STOP or queue tail that also matches stop sequences (wrk_stopseq_dev.h): advance_stop_seq / the queue's _seq kernels
    // on the frame's stop-sequence buffers, in the place and with the launch count of the tail without them
    bool stop_seqs = false;
    // DRY / the n-gram ban (wrk_dry.hip): between the penalise and the mask, dry_rows on dry_par -- in place on pen_o when
    // penalised, else on dry.out = a copy of head_o -- and the tail pushes the draw into the token window where it updates the occurrence
    // rows, under the same gate
    bool dry = false;
    // a queue tail whose prompt tokens enter the slots' contexts: behind the reset / turnover, occurrence_update (penalised)
    // and window_push (dry) once more, on io.tokens under the gate of the intake flags advance_queue wrote
    bool intake = false;
    // a QUEUE_POOL tail with a history pool: queue_history_turnover in the place of the occurrence reset
    bool history = false;
    // logit bias (wrk_bias.hip): in front of everything else, bias_rows makes bias.out = head_o biased with the rows' sets of
    // bias.par, and the penalise, the DRY copy, the mask and the pick read it where they read head_o; log-probs keep head_o
    bool biased = false;
    // classifier-free guidance (wrk_guide.hip): the step runs 2R sequences, the conditional ones [0, R) and their partners
    // [R, 2R); in front of the bias guide_rows makes guide.out [R][V] from rows r and R + r of head_o and the scales of guide.par, and the
    // whole chain and the pick run on R rows of it; log-probs keep rows [0, R) of head_o; then guide_follow, and the tail over 2R rows.
    // With a QUEUE tail: R request slots, each a pair of state slots; advance_queue_guided / queue_reset_guided are the tail
    bool guided = false;
    bool sampled() const { return pick != GREEDY; }
    bool filtered() const { return pick == FILTERED || pick == CUT; }     // the step has filter rows
    bool cut() const { return pick == CUT; }
    bool mirostat() const { return pick == MIROSTAT; }
    bool alt() const { return pick == MIROSTAT || pick == TYPICAL; }
    bool queue() const { return tail == QUEUE || tail == QUEUE_POOL; }
    bool pool() const { return tail == QUEUE_POOL; }
    // The kind's bits of GraphKey::mode, the only place they are defined: pick 24-25 and, its third bit, 30 (the first three picks keep the
    // keys they had with two bits; CUT = 5 fits the three bits, so key() is as it was), penalised 26, tail 27-28 (its third bit: key2()), log-probs 29, constrained 31 (the word is full) -- above every flag of an
    // infer job and of a runner's own (wrk_frame_common::key_bits, all below bit 24, ORed into the same word)
    uint32_t key() const {
        return ((uint32_t)pick & 3u) << 24 | ((uint32_t)pick >> 2) << 30 | (uint32_t)penalized << 26 | ((uint32_t)tail & 3u) << 27 | (uint32_t)logprobs << 29 |
               (uint32_t)constrained << 31;
    }
    // The kind's bits of GraphKey::mode2, the word that takes what key() has no room for: stop sequences 0, DRY 1, prompt intake 2,
    // history 3, biased 4, the tail's third bit (the beam tail) 5, guided 6.  0 for every kind that existed before the word did, and bit 0 alone for every
    // stop-sequence kind, so their keys compare as they always have
    uint32_t key2() const {
        return (uint32_t)stop_seqs | (uint32_t)dry << 1 | (uint32_t)intake << 2 | (uint32_t)history << 3 | (uint32_t)biased << 4 | ((uint32_t)tail >> 2) << 5 |
               (uint32_t)guided << 6;
    }
};

// ------------------------------------------------------------------ the buffer groups of a frame (Pieces of wrk_dev_group)
// Each struct is the device pointers of one feature and its layout(): the only place the sizes of its buffers are written
struct wrk_history_bufs {       // generated tokens [steps][B]
    static constexpr int DIMS = 1;              // entries
    static constexpr unsigned EXACT = 0;
    uint32_t* tokens = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(tokens, d[0] * 4 + 256); }
};
// per-sequence parameter rows the step programs read through the pointer, never baked in: generate_sample's sampler rows
// (wrk::SampleParam), next to them the top-k / min-p rows of a filtered pick (wrk::SampleFilter) or the (tau, eta, mu, typical_p) rows
// of a Mirostat / typical pick (wrk::SampleAlt): the Mirostat sampler rewrites a row's mu at every draw that counts, and the
// call reads the rows back
template <class Row> struct wrk_rows_bufs {
    static constexpr int DIMS = 1;              // sequences
    static constexpr unsigned EXACT = 0;
    Row* par = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(par, d[0] * sizeof(Row)); }
};
// generate_penalized: per-sequence occurrence rows and penalties (the step programs read the table's pointers from here); out: the
// penalised logits [B][V]
struct wrk_penalty_bufs {
    static constexpr int DIMS = 2;              // sequences, vocabulary
    static constexpr unsigned EXACT = 0;
    wrk::PenaltyParam* par = nullptr;
    float* out = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(par, d[0] * sizeof(wrk::PenaltyParam)); c.take(out, d[0] * d[1] * 4); }
};
// constrained decoding (wrk_grammar.hip).  par: the parameter block (the grammar's tables and `state`: one program serves
// any grammar and any start states); state: the sequences' automaton states, read back after the call; out [B][V]: the masked head
// output of a pick without penalties
struct wrk_grammar_bufs {
    static constexpr int DIMS = 2;              // sequences, vocabulary
    static constexpr unsigned EXACT = 2;
    wrk::GrammarParam* par = nullptr;
    uint32_t* state = nullptr;
    float* out = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(par, sizeof(wrk::GrammarParam)); c.take(state, d[0] * 4); c.take(out, d[0] * d[1] * 4); }
};
// logit bias (wrk_bias.hip).  par: the parameter block (the object's arrays and `set`: one program serves any object and any
// choice of sets); set: the sequences' set words; out [B][V]: the biased head output
struct wrk_bias_bufs {
    static constexpr int DIMS = 2;              // sequences, vocabulary
    static constexpr unsigned EXACT = 2;
    wrk::BiasParam* par = nullptr;
    uint32_t* set = nullptr;
    float* out = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(par, sizeof(wrk::BiasParam)); c.take(set, d[0] * 4); c.take(out, d[0] * d[1] * 4); }
};
// classifier-free guidance (wrk_guide.hip).  par: the guided sequences' scales (one program serves any scales); out [R][V]:
// the guided rows, which the chain reads where it read the head output
struct wrk_guide_bufs {
    static constexpr int DIMS = 2;              // guided sequences, vocabulary
    static constexpr unsigned EXACT = 2;
    float* par = nullptr;
    float* out = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(par, d[0] * 4); c.take(out, d[0] * d[1] * 4); }
};
// DRY / the n-gram ban (wrk_dry.hip).  par: the sequences' DryParam rows (window slot, values, penalty table: one program
// serves any window and any parameters); brk: the call's breaker ids; out [B][V]: the copy of the head output that a pick without
// penalties is made on; scratch u32 [B][V]: dry_rows' per-token maxima, zero between launches
struct wrk_dry_bufs {
    static constexpr int DIMS = 2;              // sequences, vocabulary
    static constexpr unsigned EXACT = 2;
    wrk::DryParam* par = nullptr;
    wrk::DryBreakers* brk = nullptr;
    float* out = nullptr;
    uint32_t* scratch = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(par, d[0] * sizeof(wrk::DryParam)); c.take(brk, sizeof(wrk::DryBreakers)); c.take(out, d[0] * d[1] * 4);
        c.take(scratch, d[0] * d[1] * 4);
    }
};
// wrk_v*_score (wrk_score.hip): targets / logprob / rank of the header rows and their slice partials [rows][SCORE_MAX_SLICES]
struct wrk_score_bufs {
    static constexpr int DIMS = 1;              // header rows
    static constexpr unsigned EXACT = 0;
    uint32_t* targets = nullptr;
    float* logprob = nullptr;
    uint32_t* rank = nullptr;
    wrk::ScorePart* part = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(targets, d[0] * 4); c.take(logprob, d[0] * 4); c.take(rank, d[0] * 4);
        c.take(part, d[0] * wrk::SCORE_MAX_SLICES * sizeof(wrk::ScorePart));
    }
};
// generate_stop (wrk_stop.hip).  par: per-sequence stop sets and end marks; flags: just_ended [cap], then the frame's live
// count, then lengths [cap]; snap_state [cap][slot floats] and snap_logits [cap][V]: slot and logits row of a sequence at the step that
// ended it
struct wrk_stop_bufs {
    static constexpr int DIMS = 3;              // sequences, floats of one sequence's state (L * (S+2) * D), vocabulary
    static constexpr unsigned EXACT = 6;
    wrk::StopParam* par = nullptr;
    uint32_t* flags = nullptr;
    float *snap_state = nullptr, *snap_logits = nullptr;
    size_t cap = 0;                             // sequences the flags are laid out for
    void layout(wrk_dev_cut& c, const size_t* d) {
        cap = d[0];
        c.take(par, d[0] * sizeof(wrk::StopParam)); c.take(flags, (2 * d[0] + 1) * 4);
        c.take(snap_state, d[0] * d[1] * 4); c.take(snap_logits, d[0] * d[2] * 4);
    }
    uint32_t* just_ended() const { return flags; }
    uint32_t* live() const { return flags + cap; }
    uint32_t* lengths() const { return flags + cap + 1; }
};
// stop sequences of generate_stop (wrk_stopseq_dev.h), per sequence: rows, tails [n][WRK_STOP_TAIL_LEN], match words
struct wrk_seq_bufs {
    static constexpr int DIMS = 1;              // sequences
    static constexpr unsigned EXACT = 0;
    wrk::StopSeqRow* rows = nullptr;
    uint32_t *tail = nullptr, *match = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(rows, d[0] * sizeof(wrk::StopSeqRow)); c.take(tail, d[0] * WRK_STOP_TAIL_LEN * 4); c.take(match, d[0] * 4);
    }
};
// generate_queue (wrk_queue.hip): slot records and started flags [slots], the control words, the prompt token pool [pool
// tokens] and everything of a request [requests], the only group with that dimension: the table and the log, and what a request carries
// for the call's features, used or not -- its mu, automaton state, bias set word, DRY values, stop sequences and match word, intake offset, pool entries
struct wrk_queue_bufs {
    static constexpr int DIMS = 3;              // slots, requests, pool tokens
    static constexpr unsigned EXACT = 0;
    wrk::QueueSlot* slots = nullptr;
    uint32_t* started = nullptr;
    wrk::QueueCtl* ctl = nullptr;
    wrk::QueueReq* reqs = nullptr;
    wrk::QueueLog* log = nullptr;
    uint32_t* pool = nullptr;
    float* mu = nullptr;
    wrk::DryParam* dry = nullptr;
    wrk::StopSeqRow* seq_rows = nullptr;
    uint32_t *gram = nullptr, *seq_match = nullptr, *from = nullptr, *bias = nullptr;
    uint32_t *start = nullptr, *save = nullptr; // one piece: save == start + request cap
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(slots, d[0] * sizeof(wrk::QueueSlot)); c.take(started, d[0] * 4); c.take(ctl, sizeof(wrk::QueueCtl));
        c.take(reqs, d[1] * sizeof(wrk::QueueReq)); c.take(log, d[1] * sizeof(wrk::QueueLog)); c.take(pool, d[2] * 4);
        c.take(mu, d[1] * 4); c.take(gram, d[1] * 4); c.take(dry, d[1] * sizeof(wrk::DryParam));
        c.take(seq_rows, d[1] * sizeof(wrk::StopSeqRow)); c.take(seq_match, d[1] * 4); c.take(from, d[1] * 4); c.take(start, 2 * d[1] * 4);
        c.take(bias, d[1] * 4);
        save = start ? start + d[1] : nullptr;
    }
    uint32_t* live() const { return &ctl->live; }
};
// what the queue's features keep per slot: the stop-sequence tails [slots][WRK_STOP_TAIL_LEN] ...
struct wrk_queue_seq_bufs {
    static constexpr int DIMS = 1;              // slots
    static constexpr unsigned EXACT = 0;
    uint32_t* tail = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(tail, d[0] * WRK_STOP_TAIL_LEN * 4); }
};
// ... and the prompt-intake flags
struct wrk_queue_intake_bufs {
    static constexpr int DIMS = 1;              // slots
    static constexpr unsigned EXACT = 0;
    uint32_t* flags = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(flags, d[0] * 4); }
};
// a guided queue: the pairs' dispatch flags [pairs] and the requests' negative prompts (offsets into the queue's token
// pool, lengths) and scales [requests]; the pairs' scale row is the guide group's
struct wrk_queue_guide_bufs {
    static constexpr int DIMS = 2;              // pairs, requests
    static constexpr unsigned EXACT = 0;
    uint32_t *pair_started = nullptr, *neg_off = nullptr, *neg_len = nullptr;
    float* scale = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(pair_started, d[0] * 4); c.take(neg_off, d[1] * 4); c.take(neg_len, d[1] * 4); c.take(scale, d[1] * 4); }
};
// a queue call with a state pool: the pool's control words and the turnover list [slots]
struct wrk_queue_state_bufs {
    static constexpr int DIMS = 1;              // slots
    static constexpr unsigned EXACT = 0;
    wrk::QueueStateCtl* ctl = nullptr;
    wrk::QueueTurn* turn = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) { c.take(ctl, sizeof(wrk::QueueStateCtl)); c.take(turn, d[0] * sizeof(wrk::QueueTurn)); }
};
// log-probs in the decode loops (wrk_logprob.hip).  par: the parameter block (the output buffers and num_top: one program
// serves any num_top); the per-step rows logprob [rows], top_ids / top_logprobs [rows][WRK_MAX_TOP_LOGPROBS], indexed
// [steps][B](, [num_top]) by a call; the slice partials and candidate keys of `batch` rows
struct wrk_logprob_bufs {
    static constexpr int DIMS = 2;              // rows, batch
    static constexpr unsigned EXACT = 0;
    wrk::LogprobParam* par = nullptr;
    float* logprob = nullptr;
    uint32_t* top_ids = nullptr;
    float* top_logprobs = nullptr;
    wrk::LogprobPart* part = nullptr;
    unsigned long long* keys = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(par, sizeof(wrk::LogprobParam)); c.take(logprob, d[0] * 4);
        c.take(top_ids, d[0] * WRK_MAX_TOP_LOGPROBS * 4); c.take(top_logprobs, d[0] * WRK_MAX_TOP_LOGPROBS * 4);
        c.take(part, wrk::logprob_part_bytes((uint32_t)d[1])); c.take(keys, wrk::logprob_key_bytes((uint32_t)d[1]));
    }
};
// beam search (wrk_beam.hip).  par / lp_par: the parameter blocks (W and the sizes; the candidate front's outputs and num_top = W);
// the slot records, the groups' stop sets, the maps and cand_ids / cand_lp [slots][WRK_MAX_BEAMS]; the front's chosen-token log-probs, slice
// partials and candidate keys; the step history [rows] x 3; inv_norm [entries]; scratch [slots][state floats]: what the permutation
// gathers into; snap [slots][state floats]: a slot's state at the step that ended it.  Both as layers of [slots of the call][slot floats]
struct wrk_beam_bufs {
    static constexpr int DIMS = 4;              // slots, history rows, inv_norm entries, floats of one sequence's state (L * (S+2) * D)
    static constexpr unsigned EXACT = 8;
    wrk::BeamParam* par = nullptr;
    wrk::LogprobParam* lp_par = nullptr;
    wrk::BeamSlot* slots = nullptr;
    wrk::BeamStop* stops = nullptr;
    uint32_t *cand_ids = nullptr, *copy_src = nullptr, *snap_map = nullptr, *done_map = nullptr, *live = nullptr, *filled = nullptr;
    float *cand_lp = nullptr, *chosen_lp = nullptr;
    wrk::LogprobPart* part = nullptr;
    unsigned long long* keys = nullptr;
    uint32_t *step_tokens = nullptr, *step_parents = nullptr;
    float *step_scores = nullptr, *inv_norm = nullptr, *scratch = nullptr, *snap = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(par, sizeof(wrk::BeamParam)); c.take(lp_par, sizeof(wrk::LogprobParam)); c.take(slots, d[0] * sizeof(wrk::BeamSlot));
        c.take(stops, d[0] * sizeof(wrk::BeamStop)); c.take(cand_ids, d[0] * WRK_MAX_BEAMS * 4); c.take(cand_lp, d[0] * WRK_MAX_BEAMS * 4);
        c.take(copy_src, d[0] * 4); c.take(snap_map, d[0] * 4); c.take(done_map, d[0] * 4); c.take(live, 4); c.take(chosen_lp, d[0] * 4);
        c.take(part, wrk::logprob_part_bytes((uint32_t)d[0])); c.take(keys, wrk::logprob_key_bytes((uint32_t)d[0]));
        c.take(step_tokens, d[1] * 4); c.take(step_parents, d[1] * 4); c.take(step_scores, d[1] * 4); c.take(inv_norm, d[2] * 4);
        c.take(scratch, d[0] * d[3] * 4); c.take(snap, d[0] * d[3] * 4); c.take(filled, d[0] * 4);
    }
    wrk::BeamBufs dev() const {
        return wrk::BeamBufs{par, slots, stops, inv_norm, cand_ids, cand_lp, step_tokens, step_parents, step_scores, copy_src, snap_map, done_map, live, filled};
    }
};
// a beam call with a context (wrk_beam.hip): the scratch of context rows that beam_context_permute gathers into -- counts
// and flags [slots][vocabulary], rings [slots][capacity], meta [slots][2], automaton states [slots].  A call without an occurrence table
// asks for vocabulary 0, one without a window for capacity 0
struct wrk_beam_ctx_bufs {
    static constexpr int DIMS = 3;              // slots, vocabulary, window capacity
    static constexpr unsigned EXACT = 0;
    float* count = nullptr;
    uint8_t* flags = nullptr;
    uint32_t *ring = nullptr, *meta = nullptr, *gram = nullptr;
    void layout(wrk_dev_cut& c, const size_t* d) {
        c.take(count, d[0] * d[1] * 4); c.take(flags, d[0] * d[1]); c.take(ring, d[0] * d[2] * 4); c.take(meta, d[0] * 2 * 4); c.take(gram, d[0] * 4);
    }
    wrk::BeamCtxScratch dev() const { return wrk::BeamCtxScratch{count, flags, ring, meta, gram}; }
};

// ------------------------------------------------------------------ frame state of a model (base of wrk_v7_model / wrk_v6_model)
struct wrk_frame_common {
    // ---- what the decode loops ask of a runner (host only: never passed to a kernel)
    virtual ~wrk_frame_common() = default;
    struct Facts { uint32_t num_vocab, num_emb, num_layer; bool has_emb; };    // has_emb: a device embedding table exists
    virtual Facts facts() const = 0;
    virtual wrk::FrameIo& io() = 0;
    // the frame of B sequences and their header rows (RWKV-7, one sequence in mode 1: also the engine); drops the programs when it grows
    virtual int32_t ensure_frame(uint32_t B, uint32_t mode) = 0;
    // one decode step of sequences [b0, b0 + B) of `st`: embed io().tokens, run the layers and the head, then wrk_enqueue_pick
    virtual int32_t enqueue_step(wrk_v7_state* st, uint32_t b0, uint32_t B, uint32_t mode, wrk_step_kind kind) = 0;
    // the runner's bits of a step program's GraphKey::mode, all below bit 24
    virtual uint32_t key_bits(uint32_t B, uint32_t mode) const { return mode; }
    // concurrent pipelines: how many the runner can run, and the frame of lane g of `groups` (lane 0 is the runner itself); the loop
    // replays lane g on lane_streams[g] and joins it through lane_events[g], which a runner of several lanes creates with the lane
    virtual uint32_t max_lanes() const { return 1; }
    virtual int32_t lane(uint32_t g, uint32_t groups, wrk_frame_common** out) { *out = this; return WRK_OK; }
    std::vector<hipStream_t> lane_streams;
    std::vector<hipEvent_t> lane_events;
    // around the timed loop of lanes [0, groups), on lane 0
    virtual void before_loop() {}
    virtual int32_t after_loop(uint32_t groups) { return WRK_OK; }

    wrk_ctx* ctx = nullptr;
    void* scratch = nullptr;
    uint32_t scratch_tokens = 0, scratch_headers = 0;
    // The side buffers of the decode-loop features and of scoring, one group each (wrk_dev_group.h): allocated by the first
    // call that needs the group, regrown by grow() before the step program is looked up, written before every call
    wrk_dev_group<wrk_history_bufs> history;
    wrk_dev_group<wrk_rows_bufs<wrk::SampleParam>> sample;
    wrk_dev_group<wrk_rows_bufs<wrk::SampleFilter>> filter;
    wrk_dev_group<wrk_rows_bufs<wrk::SampleAlt>> alt;
    wrk_dev_group<wrk_rows_bufs<wrk::SampleCut>> cut_par;      // the cut sampler's rows, next to `filter`
    wrk_dev_group<wrk_penalty_bufs> penalty;
    wrk_dev_group<wrk_grammar_bufs> grammar;
    wrk_dev_group<wrk_bias_bufs> bias;
    wrk_dev_group<wrk_guide_bufs> guide;
    wrk_dev_group<wrk_dry_bufs> dry;
    wrk_dev_group<wrk_score_bufs> score;
    wrk_dev_group<wrk_stop_bufs> stop;
    wrk_dev_group<wrk_seq_bufs> stop_seq;           // generate_stop: rows, tails and match words per sequence
    wrk_dev_group<wrk_queue_bufs> queue;
    wrk_dev_group<wrk_queue_seq_bufs> queue_seq;
    wrk_dev_group<wrk_queue_state_bufs> queue_states;
    wrk_dev_group<wrk_queue_intake_bufs> queue_intake;
    wrk_dev_group<wrk_queue_guide_bufs> queue_guide;
    wrk_dev_group<wrk_logprob_bufs> logprob;
    wrk_dev_group<wrk_beam_bufs> beam;
    wrk_dev_group<wrk_beam_ctx_bufs> beam_ctx;
    template <class F> void each_group(F&& f) {     // the one list of the groups
        f(history); f(sample); f(filter); f(alt); f(cut_par); f(penalty); f(grammar); f(bias); f(guide); f(dry); f(score); f(stop); f(stop_seq); f(queue); f(queue_seq);
        f(queue_states); f(queue_intake); f(queue_guide); f(logprob); f(beam); f(beam_ctx);
    }
    uint32_t* live_host = nullptr;              // pinned: the live counts the polled loop reads, [2 blocks][lanes]
    uint32_t live_host_cap = 0;
    std::vector<hipEvent_t> poll_events;        // [2 blocks][lanes]
    uint32_t wkv_nseq = 0;          // sequences of the job being enqueued (0: unknown): picks the WKV chunk kernel (wrk::time_mix_v7 / _v6)

    // b: tokens (generate: sequences | first sequence << 16); mode: the runner's mode and flag bits, in a decode step's key ORed
    // with wrk_step_kind::key(); nh: header rows
    // (the analogue of the reference's cached RnnJob per RnnInfo, runtime/mod.rs:110-209)
    // mode2: wrk_step_kind::key2() in a decode step's key, 0 everywhere else -- the last word compared, so keys that leave it 0 order as
    // they did without it
    struct GraphKey {
        const void* state; uint32_t b, mode, nh = 0, mode2 = 0;
        bool operator<(const GraphKey& o) const { return std::tie(state, b, mode, nh, mode2) < std::tie(o.state, o.b, o.mode, o.nh, o.mode2); }
    };
    std::map<GraphKey, wrk_program*> graphs;

    // the captured programs hold the groups' addresses: they go whenever a held group is reallocated; never inside a capture
    void drop_graphs();
    // g.ensure(want) under the one policy of wrk_dev_group, the programs dropped when a held group moves.  WRK_E_OOM / WRK_E_HIP with the
    // byte count when the allocation fails: the group is then not held, and the next call allocates again
    template <class G> int32_t grow(G& g, std::initializer_list<size_t> want) {
        const hipError_t e = g.ensure(ctx->stream, want, [this] { drop_graphs(); });
        if (e == hipSuccess) return WRK_OK;
        const int32_t code = e == hipErrorOutOfMemory ? WRK_E_OOM : WRK_E_HIP;
        if (!g.asked) return wrk_fail(ctx, code, "hipStreamSynchronize: %s", hipGetErrorString(e));
        return wrk_fail(ctx, code, "hipMalloc of %zu bytes: %s", g.asked, hipGetErrorString(e));
    }
    int32_t ensure_poll(uint32_t lanes);        // lane 0's frame: pinned live counts and events of the polled loop
    void release_common();          // destroy paths: programs, scratch and every buffer above
};

// the program cached under `key`, or -- captured from `enqueue`, which records this thread's launches -- a new one.  A program whose
// enqueue failed is destroyed and the enqueue's code returned
int32_t wrk_cached_program(wrk_ctx* ctx, std::map<wrk_frame_common::GraphKey, wrk_program*>& graphs, const wrk_frame_common::GraphKey& key,
                           const std::function<int32_t()>& enqueue, wrk_program** prog);

// upload half of a job: score targets (programs go when the slots grow), cursors, header rows, and token ids (gathered from `emb` into
// `input` with `gather`) or the embedding rows.  Read-back half: logits / arg-max / logprob + rank, then the sync; nothing inside a capture
int32_t wrk_job_upload(wrk_frame_common& f, wrk::FrameIo& io, void* input, const wrk_buf* emb, uint32_t D, const wrk_job_args& a, bool gather);
int32_t wrk_job_read_back(wrk_frame_common& f, const wrk::FrameIo& io, uint32_t V, const wrk_job_args& a);

// ------------------------------------------------------------------ the decode loops (generate_greedy ... generate_queue)
// the ABI's pick arrays, of wrk_generate_options / wrk_queue_options (wrk_pick_of) or of an entry point's own arguments, validated in
// one place (WRK_E_ARG): all three sampler arrays or none (the arg-max); penalty arrays only with a table; a table, a filter, Mirostat
// or typical only with the sampler arrays; one family of filter / Mirostat / typical per call; grammar_state only with a grammar (which
// any pick may have); bias_set only with a logit bias (which any pick may have); the DRY arrays only with a token window (which any pick
// may have), its values in their ranges.  need: what the entry point requires -- SAMPLER: the sampler arrays (generate_sample), TABLE: also the occurrence table (generate_penalized)
struct wrk_pick_args {
    const float *temperature = nullptr, *top_p = nullptr; const uint32_t* seed = nullptr;
    const float *presence = nullptr, *frequency = nullptr, *decay = nullptr; wrk_occurrence* occ = nullptr;
    const uint32_t* top_k = nullptr; const float* min_p = nullptr;      // either set: a filtered pick
    const float *mirostat_tau = nullptr, *mirostat_eta = nullptr; float* mirostat_mu = nullptr;     // tau set: a Mirostat pick; mu: in / out
    const float* typical_p = nullptr;                                   // set: a typical pick
    const wrk_grammar* grammar = nullptr; uint32_t* grammar_state = nullptr;    // grammar set: a constrained pick; grammar_state: in / out
    wrk_dry_args dry;                                                   // window set: a DRY pick
    const wrk_logit_bias* bias = nullptr; const uint32_t* bias_set = nullptr;   // bias set: a biased pick; bias_set: only read
    wrk_cut_args cut;                                                   // any set: a cut pick (with or without top_k / min_p)
    enum Need { ANY, SAMPLER, TABLE } need = ANY;
};
// the cut arrays travel in wrk_generate_options; a queue takes them beside its options (wrk_queue_cuts), whose field list is pinned
inline wrk_cut_args wrk_cut_of(const wrk_generate_options& o) {
    return {o.top_n_sigma, o.epsilon_cutoff, o.eta_cutoff, o.xtc_probability, o.xtc_threshold};
}
inline wrk_cut_args wrk_cut_of(const wrk_queue_options&) { return {}; }
inline wrk_cut_args wrk_cut_of(const wrk_queue_cuts* c) {
    return c ? wrk_cut_args{c->top_n_sigma, c->epsilon_cutoff, c->eta_cutoff, c->xtc_probability, c->xtc_threshold} : wrk_cut_args{};
}
template <class Options> wrk_pick_args wrk_pick_of(const Options& o) {
    return {o.temperature, o.top_p, o.seed, o.presence, o.frequency, o.decay, o.occ, o.top_k, o.min_p,
            o.mirostat_tau, o.mirostat_eta, o.mirostat_mu, o.typical_p, o.grammar, o.grammar_state,
            wrk_dry_args{o.window, o.dry_multiplier, o.dry_base, o.dry_allowed_length, o.no_repeat_ngram, o.dry_breakers, o.num_dry_breakers},
            o.bias, o.bias_set, wrk_cut_of(o)};
}
// the log-prob outputs of a call (wrk_generate_options / wrk_queue_options); logprob NULL: off
struct wrk_logprob_call {
    uint32_t num_top = 0; float* logprob = nullptr; uint32_t* top_ids = nullptr; float* top_logprobs = nullptr;
    bool on() const { return logprob != nullptr; }
};
bool wrk_no_graph();        // WRK_NO_GRAPH=1: the decode loops enqueue every step instead of replaying a program
// Everything of a step after the layers and the head, for sequences [b0, b0 + B) of `st`: in a guided step (B = 2R sequences)
// guide_rows first, and the chain and the pick below on the R rows of guide.out, the log-probs on rows [0, R) of head_o, guide_follow
// behind the draw updates and the tail over all B rows; the bias launch (biased: what follows reads
// its output where it read head_o or guide.out), the penalise launch (penalised), the DRY
// launches (dry: the row copy unless penalised, then dry_rows), the mask launch (constrained), the arg-max or sampler launch on the resulting row and the frame's parameters at step *counter -- neither with
// `argmax_done`: the head launch has left the arg-max in io().argmax (RWKV-7's fused greedy head, never in a constrained, a DRY or a biased step) -- with
// kind.logprobs the log-prob launches on head_o (never pen_o) and io().argmax into row
// *counter of the frame's log-prob buffers, then the tail: the occurrence update (penalised), the automaton advance (constrained) and the window push (dry) that belong to it, its advance of
// tokens / history / counter, and stop_snapshot / queue_reset / queue_turnover
int32_t wrk_enqueue_pick(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, const wrk_v7_state* st, uint32_t b0, bool argmax_done);

// wrk_v*_generate_greedy / _sample / _penalized, and with `stop` _stop: `steps` timed steps of sequences [0, B) of `st` on runner `m`,
// dealt over the lanes that bits 8-15 of mode_arg ask for (clamped to [1, min(B, m->max_lanes())]; lane g owns sequences
// [B g / groups, B (g + 1) / groups)).  Per lane, in this order -- growing a buffer drops the cached programs: ensure_frame, the
// upload of tokens / cursors / pick rows, the stop buffers, the step program {state, B | b0 << 16, key_bits | kind.key()} (none with
// WRK_NO_GRAPH=1: lane 0 enqueues every step).  Then tokens [steps][B] and last logits [B][V] come back, and with stop->opt->out_logprob
// (kind.logprobs) the log-prob rows of the steps that ran, lane by lane with the pitch copies of the tokens.
// stop: steps go out in blocks of poll_steps (0: 16), each followed by a copy of every lane's live count to pinned memory and an
// event; before block k + 2 the host waits for block k's event and stops submitting once every count is 0.  Then stop_restore, and
// lengths [B] / *steps_run come back.  With the stop-sequence arrays of stop->opt (kind.stop_seqs) every lane also gets the
// stop-sequence buffers with its sequences' rows and tails, and out_stop_match / stop_tail come back lane by lane.
// With stop->opt->guidance_scale (kind.guided) one lane runs 2B sequences -- first_tokens then guidance_first_tokens, the stop
// rows, stop-sequence rows and tails of [0, B) repeated for the partners [B, 2B) -- with B pick rows, and columns [0, B) come back
struct wrk_stop_call { const wrk_generate_options* opt; uint32_t* out_lengths; uint32_t* steps_run; };
int32_t wrk_generate(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B, uint32_t steps,
                     const wrk_pick_args& pick, uint32_t* out_tokens, float* last_logits, float* elapsed_ms, uint32_t mode_arg,
                     const wrk_stop_call* stop = nullptr);
// wrk_v*_generate_queue (tail QUEUE) / _queue_pool (QUEUE_POOL): the stop call on one lane with the queue's tail and live count
// (requests not yet ended); after the loop the log and the history rows come back and the replies are cut out of them.
// wrk_v*_generate_queue_guided (tail QUEUE, `guide` set, `guided` true): B pairs on a frame of 2B sequences -- the pick rows, the
// occurrence rows, the window, the tails and the intake flags stay B wide; the slot records, start flags, tokens and history are 2B wide
int32_t wrk_generate_queue(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                           const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, wrk_step_kind::Tail tail,
                           const wrk_queue_pool* pool, const wrk_queue_guidance* guide = nullptr, bool guided = false,
                           const wrk_queue_cuts* cuts = nullptr);
// wrk_v*_generate_queue_cut: the queue call that cuts->pool / cuts->guide select (WRK_E_ARG: cuts NULL, or both) with cuts' arrays
int32_t wrk_generate_queue_cut(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                               const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, const wrk_queue_cuts* cuts);
// wrk_v*_generate_beam (tail BEAM): the stop call's polled loop on one lane over B = G * num_beams slots with the beam tail and the count of
// LIVE slots; after the loop the DONE slots are restored from their snapshots, the records and the history rows come back and the
// hypotheses are backtracked through the parents on the host.  bc (wrk_v*_generate_beam_context; nullptr or empty: none): the
// slots' contexts -- the step runs the penalise / DRY / mask launches in front of the candidate front, and behind the state permutation
// the context permutation and the updates of the slots the step filled
int32_t wrk_generate_beam(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t G, uint32_t steps,
                          const wrk_beam_options* opt, const wrk_beam_result* out_arg, float* elapsed_ms, uint32_t mode_arg,
                          const wrk_beam_context* bc = nullptr);
