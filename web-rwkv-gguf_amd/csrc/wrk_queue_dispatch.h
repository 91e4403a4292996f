// The request queue's plain structures, the row structures a dispatch writes and the one dispatch rule, free of HIP:
// advance_queue_body (wrk_queue.hip) runs the rule on the device at every refill, wrk_queue_start (wrk_runner.hip) on the host for step
// 0 over host mirrors of the same arrays, and its host test includes this header alone.  wrk_internal.h includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wrk_hip.h"

#ifdef __HIPCC__
#define WRK_HD __host__ __device__
#else
#define WRK_HD
#endif

namespace wrk {

// ------------------------------------------------------------------ the rows of a slot (their kernels: wrk_internal.h)
struct SampleParam { float temperature, top_p; uint32_t seed, step_base; };
struct SampleFilter { uint32_t top_k; float ln_min_p; };
struct SampleAlt { float tau, eta, mu, typical_p; };
// the cut sampler's row next to SampleFilter, as wrk_cut_pack leaves it: logarithms taken once on the host in f64.
// Off: top_n_sigma 0, ln_epsilon / ln_eta -inf, xtc_probability 0 (an xtc_threshold above 0.5 is stored as probability 0)
struct SampleCut { float top_n_sigma, ln_epsilon, ln_eta, xtc_probability, ln_xtc_threshold; };
struct PenaltyParam { float* count; uint8_t* flags; const float* weight; float presence, frequency, decay; uint32_t pad; };
struct DryParam {
    uint32_t* ring; uint32_t* meta; uint32_t cap;
    uint32_t allowed, no_repeat; float multiplier;
    float pen[WRK_DRY_MAX_MATCH + 2];       // [0, WRK_DRY_MAX_MATCH]; one entry of padding keeps the row a multiple of 8 bytes
};
struct StopSeqRow;
struct QueueStateCtl;
// an owner's stop-sequence tail (wrk_stopseq_dev.h) with no draw in it
WRK_HD inline void stop_tail_clear(uint32_t* p) { for (uint32_t j = 0; j < WRK_STOP_TAIL_LEN; ++j) p[j] = WRK_STOP_TAIL_EMPTY; }

// ------------------------------------------------------------------ the queue
// R requests are served on the B slots of a state; the slot bookkeeping is device data in per-frame buffers written before every call, so
// one captured program serves any queue.  QueueReq: one request (prompt = pool[prompt_off .. + prompt_len), its pick parameters and stop
// set).  QueueSlot: what slot b is doing -- phase says what the draw of the NEXT step is: QUEUE_PROMPT a draw to discard (the step feeds a
// prompt token that is not the last), QUEUE_REPLY reply token number `reply`, QUEUE_IDLE nothing.  QueueLog: per request, as it runs.
// QUEUE_WAIT (guided queues only): the half of a pair that starts late -- `pos` more steps feed a valid id whose draws are
// ignored, then the step program resets the half's state slot and the half feeds its first token, which the dispatch left in `tokens`
enum : uint32_t { QUEUE_IDLE = 0, QUEUE_PROMPT = 1, QUEUE_REPLY = 2, QUEUE_WAIT = 3 };
static constexpr uint32_t QUEUE_NO_ENTRY = 0xFFFFFFFFu;
struct QueueReq {
    uint32_t prompt_off, prompt_len, max_new, seed;
    float temperature, top_p, presence, frequency, decay;
    uint32_t stop_count, stop_ids[WRK_MAX_STOP_TOKENS];
    uint32_t top_k; float ln_min_p;     // the request's SampleFilter row (filtered queues)
    float tau, eta, typical_p;          // the request's SampleAlt row (Mirostat / typical queues); its mu: QueueBufs::alt_mu
    float top_n_sigma, ln_epsilon, ln_eta, xtc_probability, ln_xtc_threshold;       // the request's SampleCut row (cut queues)
};
struct QueueSlot { uint32_t req, pos, reply, phase; };
struct QueueLog { uint32_t length, reason, slot, start_step; };
// init_state: [L][slot] f32 or nullptr; negative_init_state: the same for the partner halves of a guided queue
struct QueueCtl { uint32_t next_request, num_requests, live, pad; const float* init_state; const float* negative_init_state = nullptr; };
// Per slot [B]: slots, started, the rows of the call's features in their groups (nullptr: the call is without the feature), seq_tail,
// intake.  Per request [R], all the queue's own: reqs, log and what a request carries besides its QueueReq, nullptr as its rows are
struct QueueBufs {
    QueueSlot* slots; const QueueReq* reqs; const uint32_t* pool; QueueLog* log; QueueCtl* ctl;
    uint32_t* started;              // 1 when the slot took a new request in this step (written for every slot by every launch)
    SampleParam* sample_par;        // nullptr: arg-max
    PenaltyParam* pen_par;          // the slots' occurrence rows; a dispatch replaces the three values, the pointers are the slot's
    SampleFilter* filter_par;
    // Mirostat / typical.  alt_mu: request r's mu -- its start value until it is dispatched, its final value once it has ended
    // (advance_queue copies it out of the slot's row); nullptr unless Mirostat
    SampleAlt* alt_par = nullptr; float* alt_mu = nullptr;
    // constrained queues: the slots' automaton state words and request r's state, start and final value exactly as alt_mu
    uint32_t *gram_state = nullptr, *gram_req = nullptr;
    // queues with a token window: the slots' rows and request r's values and table (its ring / meta / cap are not read)
    DryParam* dry_par = nullptr; const DryParam* dry_req = nullptr;
    // queues with stop sequences: request r's sequences; the slot's tail [B][WRK_STOP_TAIL_LEN]; request r's match word
    // (NONE until a stop ends it); all three or none
    const StopSeqRow* seq_rows = nullptr; uint32_t *seq_tail = nullptr, *seq_match = nullptr;
    // prompt intake: ctx_from: the index of request r's first prompt token that enters the slot's context; intake: 1 when
    // the token this launch wrote into tokens[b] is such a prompt token (written for every slot by every launch, as started)
    const uint32_t* ctx_from = nullptr; uint32_t* intake = nullptr;
    // biased queues: the slots' bias set words and request r's (only read: a bias has no state)
    uint32_t *bias_set = nullptr, *bias_req = nullptr;
    // guided queues, all four or none: request r's negative prompt pool[neg_off[r] .. + neg_len[r]) (length 0: none) and
    // its scale; the pairs' scale row [B], the `guide` group's parameter row.  With them slots / started are [2B] -- pair b is the records
    // b (conditional half) and B + b (partner) -- and pair_started [B] is 1 when the pair took a request in this step (written for every
    // pair by every launch, as started): the flag of the occurrence reset, which stays B wide
    const uint32_t *neg_off = nullptr, *neg_len = nullptr; const float* scale_req = nullptr; float* scale = nullptr;
    uint32_t* pair_started = nullptr;
    // cut queues: the slots' SampleCut rows, next to filter_par
    SampleCut* cut_par = nullptr;
};
// A state pool under the queue.  QueueTurn: one slot that ended in the step -- `save` the entry its state goes to,
// `started` / `start` as started[slot] and the entry the slot's next request begins from; QUEUE_NO_ENTRY: none
struct QueueTurn { uint32_t slot, save, started, start; };
struct QueueStateBufs {
    const uint32_t *start, *save;   // [R]: the requests' entries
    QueueStateCtl* sctl;
    QueueTurn* turn;                // [B]: written by advance_queue_pool at position (ended slots before this one), no atomics
    // a call with a history pool: queue_history_turnover takes the place of the occurrence reset and of the dispatch's window reset
    bool history = false;
};

// THE dispatch rule: request r goes to slot b and its first prompt token p_0 is fed at step first_step.  The slot feeds p_0 .. p_{n-1}
// on steps first_step .. first_step + n - 1 and the draw of the last of them is reply token 0, so the sampler's step base is
// first_step + n - 1 and reply token j has sampler step j wherever and whenever the request runs.  Writes, through the arrays handed in
// and nothing else: the slot record, p_0, the intake flag, the slot's sampler / filter / cut / alt rows (mu from alt_mu[r]), its automaton
// state, its bias set word, the values and table of its DRY row, an empty stop tail, the three values of its penalty row, the request's log entry and,
// with a pool, turn[turn_at] = {b, save, 1, start[r]}.  The slot's own pointers -- occurrence row, window ring / meta / cap -- are never
// written.  Returns whether the caller is to set the slot's window to length 0 (the two words behind DryParam::meta): with a window,
// unless a history pool's turnover sets it
WRK_HD inline bool queue_dispatch(const QueueBufs& Q, uint32_t* tokens, uint32_t r, uint32_t b, uint32_t first_step, const QueueStateBufs* P,
                                  uint32_t turn_at = 0, uint32_t save = QUEUE_NO_ENTRY) {
    const QueueReq* q = Q.reqs + r;
    tokens[b] = Q.pool[q->prompt_off];
    if (Q.sample_par) Q.sample_par[b] = SampleParam{q->temperature, q->top_p, q->seed, first_step + q->prompt_len - 1};
    if (Q.filter_par) Q.filter_par[b] = SampleFilter{q->top_k, q->ln_min_p};
    if (Q.cut_par) Q.cut_par[b] = SampleCut{q->top_n_sigma, q->ln_epsilon, q->ln_eta, q->xtc_probability, q->ln_xtc_threshold};
    if (Q.alt_par) Q.alt_par[b] = SampleAlt{q->tau, q->eta, Q.alt_mu ? Q.alt_mu[r] : 0.0f, q->typical_p};
    if (Q.gram_req) Q.gram_state[b] = Q.gram_req[r];
    if (Q.bias_req) Q.bias_set[b] = Q.bias_req[r];
    if (Q.dry_par) {
        DryParam* dp = Q.dry_par + b;
        const DryParam* dq = Q.dry_req + r;
        dp->allowed = dq->allowed; dp->no_repeat = dq->no_repeat; dp->multiplier = dq->multiplier;
        for (uint32_t m = 0; m <= WRK_DRY_MAX_MATCH; ++m) dp->pen[m] = dq->pen[m];
    }
    if (Q.seq_tail) stop_tail_clear(Q.seq_tail + (size_t)b * WRK_STOP_TAIL_LEN);
    if (Q.pen_par) { Q.pen_par[b].presence = q->presence; Q.pen_par[b].frequency = q->frequency; Q.pen_par[b].decay = q->decay; }
    Q.log[r] = QueueLog{0u, 3u, b, first_step};
    if (P) P->turn[turn_at] = QueueTurn{b, save, 1u, P->start[r]};
    Q.slots[b] = QueueSlot{r, 0u, 0u, q->prompt_len == 1 ? QUEUE_REPLY : QUEUE_PROMPT};
    if (Q.intake) Q.intake[b] = Q.ctx_from[r] == 0u;
    return Q.dry_par && !(P && P->history);
}

// THE dispatch rule of a guided queue: request r goes to pair b of B -- slot records, tokens and state slots b and B + b --
// and step f is the first the pair runs for it.  With n the prompt's and m the negative prompt's length and L = max(n, m), the
// conditional half feeds p_0 at step f + L - n and the partner q_0 at step f + L - m, so both feed their last prompt token at step
// f + L - 1, whose draw is reply token 0: the sampler's step base is f + L - 1, and start_step = f + L - n stays "the step that fed p_0".
// Writes everything queue_dispatch writes for (r, b, first_step f + L - n) -- the pair's pick rows are the conditional request's -- and
// then: a conditional half that starts late gets the record {r, L - n, 0, QUEUE_WAIT} and no intake flag (p_0 stays in tokens[b], a
// valid id, until it is fed for good); the partner's record is QUEUE_IDLE when m == 0 (tokens[B + b] stays: neither reset nor fed), else
// q_0 goes to tokens[B + b] and the record is {r, L - m, 0, QUEUE_WAIT} or, on time, {r, 0, 0, REPLY if m == 1 else PROMPT}; the pair's
// scale.  start_cond / start_part: the half feeds its first token at step f itself -- its state slot is to be set to its start state
// in front of step f; a half in QUEUE_WAIT is reset by the step that ends its wait.  wipe: queue_dispatch's answer
struct QueuePairStart { bool wipe; uint32_t start_cond, start_part; };
WRK_HD inline QueuePairStart queue_dispatch_guided(const QueueBufs& Q, uint32_t* tokens, uint32_t r, uint32_t b, uint32_t B, uint32_t f) {
    const uint32_t n = Q.reqs[r].prompt_len, m = Q.neg_len[r], L = n > m ? n : m;
    const bool wipe = queue_dispatch(Q, tokens, r, b, f + (L - n), nullptr);
    if (L > n) {
        Q.slots[b] = QueueSlot{r, L - n, 0u, QUEUE_WAIT};
        if (Q.intake) Q.intake[b] = 0u;
    }
    if (m == 0) {
        Q.slots[B + b] = QueueSlot{r, 0u, 0u, QUEUE_IDLE};
    } else {
        tokens[B + b] = Q.pool[Q.neg_off[r]];
        Q.slots[B + b] = L > m ? QueueSlot{r, L - m, 0u, QUEUE_WAIT} : QueueSlot{r, 0u, 0u, m == 1 ? QUEUE_REPLY : QUEUE_PROMPT};
    }
    Q.scale[b] = Q.scale_req[r];
    return QueuePairStart{wipe, L == n ? 1u : 0u, m != 0 && L == m ? 1u : 0u};
}

}  // namespace wrk
