// A request queue in the decode loops for gfx950.  R requests of different prompt and reply lengths are served on the
// B slots of a state inside one call: a slot whose request ends is reset and takes the next request in the same step program, so no
// slot waits for the longest reply of a batch.  A slot is a fixed-size recurrent state plus one "next token" word, so a refill is a
// fill of that state and another token in io.tokens; a prompt is taken in at decode rate by feeding its tokens in place of the draws.
//
//   advance_queue   takes advance_tokens' place in a queue program: one thread owns a slot, pops the next prompt token or takes the
//                   draw, checks the stop set and max_new, deals the next requests to the slots that ended (exclusive scan over the slot
//                   index from one next_request word) by queue_dispatch (wrk_queue_dispatch.h) -- the one rule for "request r goes to
//                   slot b, p_0 fed at step f", which the host runs for step 0 too -- and moves the step counter last
//   queue_reset     grid (layer x slice, slot): every workgroup reads started[b] and leaves when it is 0; else zero fill / init_state
//                   copy of the slot, and a second small grid for the slot's occurrence row when the program is penalised
//   advance_queue_pool, queue_turnover   their places in the programs of a call with a state pool: the same advance body
//                   also lists the slots that ended; one (layer x slice) grid, whatever B, saves each listed slot's state to its
//                   request's pool entry and then fills the slot from the next request's entry, init_state or zeros
//   queue_history_turnover   in the programs of a pool call with a history pool, and behind wrk_history_pool_put / _get:
//                   the occurrence reset's place; one grid over the vocabulary and the largest ring walks the same turnover list, saves
//                   each listed slot's occurrence row and token window to its request's history entry and then sets them from the
//                   next request's entry, or to the reset
//   advance_queue_guided, queue_reset_guided   their places in the programs of a guided queue: a request slot is a pair of
//                   state slots, the conditional half and its partner, which takes the request's negative prompt in beside it; the
//                   advance schedules both halves so that they end their prompts in the same step, and the reset runs over 2B slots,
//                   each half set to its own start state directly in front of the step that feeds its first token
//
// started[b] is written by EVERY advance_queue launch for every slot, so the flag a reset launch reads was written by the launch in front
// of it in the same stream; nothing has to clear it.  Plain vector stores only; no atomics; no kernel waits on another.
#include "wrk_device.h"
#include "wrk_runner.h"
#include "wrk_stopseq_dev.h"

namespace wrk {

static constexpr uint32_t QUEUE_THREADS = 256;
static constexpr uint32_t QUEUE_CHUNK = QUEUE_THREADS * 4;     // floats a workgroup moves per pass (16 bytes per thread)
static constexpr uint32_t QUEUE_WAVES = QUEUE_THREADS / 64;
static constexpr uint32_t QUEUE_WINDOW_TILES = (WRK_MAX_TOKEN_WINDOW + QUEUE_CHUNK - 1) / QUEUE_CHUNK;

// slots are owned by the threads of ONE workgroup (B <= 256, as advance_stop).  POOL (advance_queue_pool_kernel): the slots that ended
// also go into the step's turnover list, at the position the scan below gives them.  SEQ (the _seq kernels): a reply draw
// goes through stop_seq_step (wrk_stopseq_dev.h) with the request's stop set and its StopSeqRow and enters the slot's tail; a match ends
// the request as a stop token does and leaves its match word.  What a slot that takes a request starts with is queue_dispatch's
template <bool POOL, bool SEQ>
__device__ __forceinline__ void advance_queue_body(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                   uint32_t* __restrict__ history, uint32_t* __restrict__ counter, const QueueBufs& Q,
                                                   const QueueStateBufs& P, uint32_t b) {
    __shared__ uint32_t wave_ended[QUEUE_WAVES];
    const uint32_t step = *counter;
    const uint32_t next = Q.ctl->next_request, live = Q.ctl->live, num_requests = Q.ctl->num_requests;
    const uint32_t i = threadIdx.x, lane = i & 63u, wave = i >> 6;
    int ended = 0;
    uint32_t take = 0;                          // the token this launch writes into tokens[i] is a prompt token that enters the context
    QueueSlot s{0u, 0u, 0u, QUEUE_IDLE};
    if (i < b) {
        s = Q.slots[i];
        const uint32_t y = drawn[i];
        history[(size_t)step * b + i] = y;     // a prompt-phase or idle draw too: the host cuts the replies out by the log
        if (s.phase == QUEUE_PROMPT) {
            const QueueReq* r = Q.reqs + s.req;
            s.pos += 1;
            tokens[i] = Q.pool[r->prompt_off + s.pos];
            if (Q.ctx_from) take = s.pos >= Q.ctx_from[s.req];
            if (s.pos + 1 == r->prompt_len) s.phase = QUEUE_REPLY;
        } else if (s.phase == QUEUE_REPLY) {
            const QueueReq* r = Q.reqs + s.req;
            tokens[i] = y;
            const uint32_t n = r->stop_count < WRK_MAX_STOP_TOKENS ? r->stop_count : WRK_MAX_STOP_TOKENS;
            int hit = 0;
            if (SEQ) {
                uint32_t* tp = Q.seq_tail + (size_t)i * STOP_TAIL;
                StopTail tail = stop_tail_load(tp);
                const uint32_t match = stop_seq_step(tail, y, Q.seq_rows + s.req, r->stop_ids, n);
                stop_tail_store(tp, tail);
                hit = match != WRK_STOP_MATCH_NONE;
                if (hit) Q.seq_match[s.req] = match;
            } else {
                for (uint32_t k = 0; k < n; ++k) hit |= (r->stop_ids[k] == y);
            }
            s.reply += 1;
            Q.log[s.req].length = s.reply;
            const uint32_t reason = hit ? 1u : (s.reply == r->max_new ? 2u : 0u);
            if (reason) {
                Q.log[s.req].reason = reason; ended = 1;
                if (Q.alt_mu) Q.alt_mu[s.req] = Q.alt_par[i].mu;     // the sampler of this step has counted the last draw
                if (Q.gram_req) Q.gram_req[s.req] = Q.gram_state[i];    // and grammar_advance, in front of this launch, has moved on it
            }
        }                                       // idle: tokens[i] stays, a valid id keeps flowing through the embedding gather
    }
    // exclusive scan of `ended` over the slot index: in-wave by ballot, across the four waves through LDS
    const unsigned long long mask = __ballot(ended);
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_ended[wave] = (uint32_t)__popcll(mask);
    __syncthreads();                            // also orders every read of *counter and *ctl before their update
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < QUEUE_WAVES; ++w) {
        if (w < wave) before += wave_ended[w];
        total += wave_ended[w];
    }
    if (i < b) {
        uint32_t started = 0, save = QUEUE_NO_ENTRY;
        if (ended) {
            if (POOL) save = P.save[s.req];
            s.phase = QUEUE_IDLE;
            started = next + before + rank < num_requests;
        }
        if (started) {
            // the next step feeds p_0 (a request is dispatched once: its own mu and automaton state still hold their start values).  An
            // empty window: window_push, in front of this launch, has pushed the last draw of the request that ended, and dry_rows of the
            // next step reads it next; with a history pool queue_history_turnover, behind this launch, saves the window, then sets it
            if (queue_dispatch(Q, tokens, next + before + rank, i, step + 1, POOL ? &P : nullptr, before + rank, save)) {
                uint32_t* meta = Q.dry_par[i].meta;
                meta[0] = meta[1] = 0u;
            }
        } else {
            if (POOL && ended) P.turn[before + rank] = QueueTurn{i, save, 0u, QUEUE_NO_ENTRY};
            Q.slots[i] = s;
            if (Q.intake) Q.intake[i] = take;
        }
        Q.started[i] = started;
    }
    if (i == 0) {
        if (total) { Q.ctl->next_request = next + total; Q.ctl->live = live - total; }
        if (POOL) P.sctl->turn_count = total;
        *counter = step + 1;
    }
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                      uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                      const QueueBufs Q, uint32_t b) {
    advance_queue_body<false, false>(drawn, tokens, history, counter, Q, QueueStateBufs{}, b);
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_seq_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                          uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                          const QueueBufs Q, uint32_t b) {
    advance_queue_body<false, true>(drawn, tokens, history, counter, Q, QueueStateBufs{}, b);
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_pool_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                           uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                           const QueueBufs Q, const QueueStateBufs P, uint32_t b) {
    advance_queue_body<true, false>(drawn, tokens, history, counter, Q, P, b);
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_pool_seq_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                               uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                               const QueueBufs Q, const QueueStateBufs P, uint32_t b) {
    advance_queue_body<true, true>(drawn, tokens, history, counter, Q, P, b);
}

// A guided queue: B <= QUEUE_THREADS / 2 pairs, thread i < B owns pair i -- the slot records, tokens and start flags i
// (the conditional half) and B + i (its partner).  Either half pops its prompt tokens or counts its wait down; the step that ends a wait
// raises the half's start flag, so that the reset behind this launch sets its state slot directly in front of the step that feeds its
// first token (which queue_dispatch_guided left in `tokens`).  The conditional half's reply draw -- made on the guided row, and copied to
// row B + i by guide_follow in front of this launch -- is fed to both halves, checked and counted exactly as advance_queue_body does; the
// end releases both halves and the pair takes the next request in the same step, by the same scan.  started [2B] and pair_started [B]
// are written for every slot and pair by every launch
template <bool SEQ>
__device__ __forceinline__ void advance_queue_guided_body(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                          uint32_t* __restrict__ history, uint32_t* __restrict__ counter, const QueueBufs& Q,
                                                          uint32_t b) {
    __shared__ uint32_t wave_ended[QUEUE_WAVES];
    const uint32_t step = *counter;
    const uint32_t next = Q.ctl->next_request, live = Q.ctl->live, num_requests = Q.ctl->num_requests;
    const uint32_t i = threadIdx.x, lane = i & 63u, wave = i >> 6;
    int ended = 0;
    uint32_t take = 0, start_c = 0, start_p = 0;
    QueueSlot s{0u, 0u, 0u, QUEUE_IDLE}, p{0u, 0u, 0u, QUEUE_IDLE};
    if (i < b) {
        s = Q.slots[i];
        p = Q.slots[b + i];
        const uint32_t y = drawn[i];
        history[(size_t)step * 2u * b + i] = y;         // 2B wide, as a guided stop program's: the host cuts the replies out of columns [0, B)
        history[(size_t)step * 2u * b + b + i] = drawn[b + i];
        // the partner first: its phases never decide anything
        if (p.phase == QUEUE_WAIT) {
            p.pos -= 1;
            if (p.pos == 0) { start_p = 1; p.phase = Q.neg_len[p.req] == 1 ? QUEUE_REPLY : QUEUE_PROMPT; }
        } else if (p.phase == QUEUE_PROMPT) {
            p.pos += 1;
            tokens[b + i] = Q.pool[Q.neg_off[p.req] + p.pos];
            if (p.pos + 1 == Q.neg_len[p.req]) p.phase = QUEUE_REPLY;
        } else if (p.phase == QUEUE_REPLY) {
            tokens[b + i] = y;
        }                                               // idle: tokens[b + i] stays
        if (s.phase == QUEUE_WAIT) {
            s.pos -= 1;
            if (s.pos == 0) {
                start_c = 1;
                s.phase = Q.reqs[s.req].prompt_len == 1 ? QUEUE_REPLY : QUEUE_PROMPT;
                if (Q.ctx_from) take = Q.ctx_from[s.req] == 0u;     // p_0, in tokens[i] since the dispatch, is fed by the next step
            }
        } else if (s.phase == QUEUE_PROMPT) {
            const QueueReq* r = Q.reqs + s.req;
            s.pos += 1;
            tokens[i] = Q.pool[r->prompt_off + s.pos];
            if (Q.ctx_from) take = s.pos >= Q.ctx_from[s.req];
            if (s.pos + 1 == r->prompt_len) s.phase = QUEUE_REPLY;
        } else if (s.phase == QUEUE_REPLY) {
            const QueueReq* r = Q.reqs + s.req;
            tokens[i] = y;
            const uint32_t n = r->stop_count < WRK_MAX_STOP_TOKENS ? r->stop_count : WRK_MAX_STOP_TOKENS;
            int hit = 0;
            if (SEQ) {
                uint32_t* tp = Q.seq_tail + (size_t)i * STOP_TAIL;
                StopTail tail = stop_tail_load(tp);
                const uint32_t match = stop_seq_step(tail, y, Q.seq_rows + s.req, r->stop_ids, n);
                stop_tail_store(tp, tail);
                hit = match != WRK_STOP_MATCH_NONE;
                if (hit) Q.seq_match[s.req] = match;
            } else {
                for (uint32_t k = 0; k < n; ++k) hit |= (r->stop_ids[k] == y);
            }
            s.reply += 1;
            Q.log[s.req].length = s.reply;
            const uint32_t reason = hit ? 1u : (s.reply == r->max_new ? 2u : 0u);
            if (reason) {
                Q.log[s.req].reason = reason; ended = 1;
                if (Q.alt_mu) Q.alt_mu[s.req] = Q.alt_par[i].mu;
                if (Q.gram_req) Q.gram_req[s.req] = Q.gram_state[i];
            }
        }
    }
    const unsigned long long mask = __ballot(ended);
    const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_ended[wave] = (uint32_t)__popcll(mask);
    __syncthreads();                            // also orders every read of *counter and *ctl before their update
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < QUEUE_WAVES; ++w) {
        if (w < wave) before += wave_ended[w];
        total += wave_ended[w];
    }
    if (i < b) {
        uint32_t dealt = 0;
        if (ended) {
            s.phase = QUEUE_IDLE;
            p.phase = QUEUE_IDLE;
            dealt = next + before + rank < num_requests;
        }
        if (dealt) {
            const QueuePairStart ps = queue_dispatch_guided(Q, tokens, next + before + rank, i, b, step + 1);
            if (ps.wipe) {
                uint32_t* meta = Q.dry_par[i].meta;
                meta[0] = meta[1] = 0u;
            }
            start_c = ps.start_cond; start_p = ps.start_part;
        } else {
            Q.slots[i] = s;
            Q.slots[b + i] = p;
            if (Q.intake) Q.intake[i] = take;
        }
        Q.started[i] = start_c;
        Q.started[b + i] = start_p;
        Q.pair_started[i] = dealt;
    }
    if (i == 0) {
        if (total) { Q.ctl->next_request = next + total; Q.ctl->live = live - total; }
        *counter = step + 1;
    }
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_guided_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                             uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                             const QueueBufs Q, uint32_t b) {
    advance_queue_guided_body<false>(drawn, tokens, history, counter, Q, b);
}

__global__ void __launch_bounds__(QUEUE_THREADS) advance_queue_guided_seq_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                                 uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                                 const QueueBufs Q, uint32_t b) {
    advance_queue_guided_body<true>(drawn, tokens, history, counter, Q, b);
}

struct QueueResetArgs {
    float* state;               // [L][num_batch][slot] f32
    const uint32_t* started;
    const QueueCtl* ctl;
    uint32_t layers, slices, num_batch, b0, vec;
    size_t slot;                // (S + 2) * D
};

// GUIDED (queue_reset_state_guided_kernel): the grid's y runs over the 2 * pairs state slots of a guided queue, and a partner slot
// (y >= pairs) starts from negative_init_state
template <bool GUIDED>
__device__ __forceinline__ void queue_reset_state_body(const QueueResetArgs& A, uint32_t pairs) {
    const uint32_t b = blockIdx.y;
    if (A.started[b] == 0) return;
    const uint32_t l = blockIdx.x / A.slices, part = blockIdx.x - l * A.slices;
    float* dst = A.state + ((size_t)l * A.num_batch + A.b0 + b) * A.slot;
    const float* init = GUIDED && b >= pairs ? A.ctl->negative_init_state : A.ctl->init_state;
    const float* src = init ? init + (size_t)l * A.slot : nullptr;
    const size_t n = A.slot;
    if (A.vec && (((uintptr_t)src) & 15u) == 0) {
        for (size_t i = (size_t)part * QUEUE_CHUNK + threadIdx.x * 4; i < n; i += (size_t)A.slices * QUEUE_CHUNK)
            *(f32x4*)(dst + i) = src ? *(const f32x4*)(src + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
        for (size_t i = (size_t)part * QUEUE_THREADS + threadIdx.x; i < n; i += (size_t)A.slices * QUEUE_THREADS) dst[i] = src ? src[i] : 0.0f;
    }
}

__global__ void __launch_bounds__(QUEUE_THREADS) queue_reset_state_kernel(const QueueResetArgs A) { queue_reset_state_body<false>(A, 0u); }

__global__ void __launch_bounds__(QUEUE_THREADS) queue_reset_state_guided_kernel(const QueueResetArgs A, uint32_t pairs) {
    queue_reset_state_body<true>(A, pairs);
}

// Pool programs: queue_reset_state_kernel's place.  Workgroup (layer, slice) walks the step's turnover list; a thread moves the same
// 16-byte elements of every listed slot, and for one element loads the slot, stores it to the save entry and only then stores the slot's
// new value, so a slot that ends and restarts in one step is saved before it is overwritten with no ordering between workgroups.  The
// entries read and the entries written in one step are disjoint (host validation), and a slot is listed once
struct QueueTurnArgs {
    float* state;               // [L][num_batch][slot] f32
    const QueueStateCtl* sctl;
    const QueueTurn* turn;
    const QueueCtl* ctl;
    uint32_t layers, slices, num_batch, b0;
    size_t slot;                // (S + 2) * D, a multiple of 4
};

__global__ void __launch_bounds__(QUEUE_THREADS) queue_turnover_kernel(const QueueTurnArgs A) {
    const QueueStateCtl sc = *A.sctl;
    if (sc.turn_count == 0) return;
    const uint32_t l = blockIdx.x / A.slices, part = blockIdx.x - l * A.slices;
    const float* init = A.ctl->init_state;
    const size_t n = A.slot, entry = (size_t)A.layers * A.slot;
    for (uint32_t t = 0; t < sc.turn_count; ++t) {
        const QueueTurn e = A.turn[t];
        float* cur = A.state + ((size_t)l * A.num_batch + A.b0 + e.slot) * A.slot;
        float* save = e.save != QUEUE_NO_ENTRY ? sc.states + (size_t)e.save * entry + (size_t)l * A.slot : nullptr;
        const float* src = e.start != QUEUE_NO_ENTRY ? sc.states + (size_t)e.start * entry + (size_t)l * A.slot
                                                     : (init ? init + (size_t)l * A.slot : nullptr);
        if (!save && !e.started) continue;
        for (size_t i = (size_t)part * QUEUE_CHUNK + threadIdx.x * 4; i < n; i += (size_t)A.slices * QUEUE_CHUNK) {
            if (save) *(f32x4*)(save + i) = *(const f32x4*)(cur + i);
            if (e.started) *(f32x4*)(cur + i) = src ? *(const f32x4*)(src + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
}

// occurrence row of a slot that starts a request: count = 0, present cleared, banned kept.  ceil(v / 1024) workgroups per slot, thread
// tid owns the 4 elements at 4 * tid (VEC: rows start 16-byte aligned, v % 4 == 0, as wrk_penalty.hip) or tid + 256 * j
template <bool VEC>
__global__ void __launch_bounds__(QUEUE_THREADS) queue_reset_occurrence_kernel(uint32_t v, const PenaltyParam* __restrict__ par,
                                                                               const uint32_t* __restrict__ started) {
    const uint32_t b = blockIdx.y, tid = threadIdx.x;
    if (started[b] == 0) return;
    const PenaltyParam p = par[b];
    const uint32_t a = blockIdx.x * QUEUE_CHUNK;
    if (VEC) {
        const uint32_t i = a + tid * 4;
        if (i >= v) return;
        *(f32x4*)(p.count + i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t* f = (uint32_t*)(p.flags + i);
        *f = *f & 0x02020202u;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t i = a + j * QUEUE_THREADS + tid;
            if (i < v) { p.count[i] = 0.0f; p.flags[i] = p.flags[i] & 2u; }
        }
    }
}

// Call with a history pool: queue_reset_occurrence_kernel's place, and the window reset's.  Workgroups [0, row_tiles) own 1024 elements
// of the occurrence rows each (thread tid the 4 at 4 * tid when VEC, else tid + 256 * j); the QUEUE_WINDOW_TILES workgroups behind them
// 1024 ring elements each -- the largest ring, whatever the window's capacity, which is data -- and the first of them, in thread 0, the
// window's (length, position) words.  Every thread walks the turnover list and, per element of
// a listed slot, loads the slot, stores it to the save entry and only then stores the slot's new value: a slot that ends and restarts
// in one step is saved before it is overwritten with no ordering between workgroups.  The entries read and written in one step are
// disjoint (host validation), a slot is listed once, and a ring is copied whole, so no element depends on the meta words
struct QueueHistArgs {
    const QueueStateCtl* sctl;
    const QueueTurn* turn;
    const PenaltyParam* pen;    // the slots' occurrence rows, or nullptr
    const DryParam* dry;        // the slots' windows, or nullptr
    uint32_t v, row_tiles;
};

template <bool VEC>
__global__ void __launch_bounds__(QUEUE_THREADS) queue_history_turnover_kernel(const QueueHistArgs A) {
    const QueueStateCtl sc = *A.sctl;
    if (sc.turn_count == 0) return;
    const QueueHistory H = sc.hist;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x < A.row_tiles) {
        if (!A.pen || !H.count) return;
        const uint32_t a = blockIdx.x * QUEUE_CHUNK, v = A.v;
        for (uint32_t t = 0; t < sc.turn_count; ++t) {
            const QueueTurn e = A.turn[t];
            const bool save = e.save != QUEUE_NO_ENTRY, load = e.started && e.start != QUEUE_NO_ENTRY;
            if (!save && !e.started) continue;
            const PenaltyParam p = A.pen[e.slot];
            float* sc_c = save ? H.count + (size_t)e.save * v : nullptr;
            uint8_t* sc_f = save ? H.flags + (size_t)e.save * v : nullptr;
            const float* ld_c = load ? H.count + (size_t)e.start * v : nullptr;
            const uint8_t* ld_f = load ? H.flags + (size_t)e.start * v : nullptr;
            if (VEC) {
                const uint32_t i = a + tid * 4;
                if (i >= v) continue;
                const f32x4 c = *(const f32x4*)(p.count + i);
                const uint32_t f = *(const uint32_t*)(p.flags + i);
                if (save) { *(f32x4*)(sc_c + i) = c; *(uint32_t*)(sc_f + i) = f & 0x01010101u; }
                if (e.started) {
                    *(f32x4*)(p.count + i) = load ? *(const f32x4*)(ld_c + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    *(uint32_t*)(p.flags + i) = (f & 0x02020202u) | (load ? *(const uint32_t*)(ld_f + i) & 0x01010101u : 0u);
                }
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t i = a + j * QUEUE_THREADS + tid;
                    if (i >= v) continue;
                    const float c = p.count[i];
                    const uint8_t f = p.flags[i];
                    if (save) { sc_c[i] = c; sc_f[i] = f & 1u; }
                    if (e.started) {
                        p.count[i] = load ? ld_c[i] : 0.0f;
                        p.flags[i] = (uint8_t)((f & 2u) | (load ? ld_f[i] & 1u : 0u));
                    }
                }
            }
        }
        return;
    }
    if (!A.dry || !H.ring) return;
    const uint32_t w = blockIdx.x - A.row_tiles;
    for (uint32_t t = 0; t < sc.turn_count; ++t) {
        const QueueTurn e = A.turn[t];
        const bool save = e.save != QUEUE_NO_ENTRY, load = e.started && e.start != QUEUE_NO_ENTRY;
        if (!save && !e.started) continue;
        const DryParam* p = A.dry + e.slot;
        uint32_t* ring = p->ring;
        const uint32_t cap = p->cap < H.cap ? p->cap : H.cap;      // equal (host validation); the window's capacity is data
        uint32_t* sv = save ? H.ring + (size_t)e.save * cap : nullptr;
        const uint32_t* ld = load ? H.ring + (size_t)e.start * cap : nullptr;
        if (save || load) {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = w * QUEUE_CHUNK + j * QUEUE_THREADS + tid;
                if (i >= cap) continue;
                const uint32_t x = ring[i];
                if (save) sv[i] = x;
                if (load) ring[i] = ld[i];
            }
        }
        if (w == 0 && tid == 0) {
            uint32_t* m = p->meta;
            const uint32_t len = m[0], pos = m[1];
            if (save) { H.meta[(size_t)e.save * 2] = len; H.meta[(size_t)e.save * 2 + 1] = pos; }
            if (e.started) {
                m[0] = load ? H.meta[(size_t)e.start * 2] : 0u;
                m[1] = load ? H.meta[(size_t)e.start * 2 + 1] : 0u;
            }
        }
    }
}

void queue_history_turnover(hipStream_t s, uint32_t v, const QueueStateCtl* sctl, const QueueTurn* turn, const PenaltyParam* pen,
                            const DryParam* dry) {
    QueueHistArgs A{sctl, turn, pen, dry, v, pen ? (v + QUEUE_CHUNK - 1) / QUEUE_CHUNK : 0u};
    const uint32_t grid = A.row_tiles + (dry ? QUEUE_WINDOW_TILES : 0u);
    if (grid == 0) return;
    if (v % 4 == 0) queue_history_turnover_kernel<true><<<grid, QUEUE_THREADS, 0, s>>>(A);
    else queue_history_turnover_kernel<false><<<grid, QUEUE_THREADS, 0, s>>>(A);
}

void advance_queue(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q, uint32_t b) {
    // a queue with stop sequences has all three of their buffers (queue_bufs)
    if (q.seq_rows) advance_queue_seq_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, b);
    else advance_queue_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, b);
}

// slices of a layer's slot: layers * slices workgroups come to about two per CU, so that one starting request's fill (13 MB at the
// 1.5B shape) runs on the whole chip, and no slice is smaller than one pass
static uint32_t queue_slices(const QueueGeom& g, uint32_t per_pass, int num_cu) {
    const uint32_t max_slices = (uint32_t)((g.slot + per_pass - 1) / per_pass);
    const uint32_t want = (2u * (uint32_t)num_cu + g.layers - 1) / g.layers;
    return want < 1 ? 1 : (want > max_slices ? max_slices : want);
}

static void queue_reset_occurrence(hipStream_t s, const QueueGeom& g, const QueueBufs& q, uint32_t b) {
    if (!q.pen_par || g.v == 0) return;
    const dim3 grid((g.v + QUEUE_CHUNK - 1) / QUEUE_CHUNK, b);
    if (g.v % 4 == 0) queue_reset_occurrence_kernel<true><<<grid, QUEUE_THREADS, 0, s>>>(g.v, q.pen_par, q.started);
    else queue_reset_occurrence_kernel<false><<<grid, QUEUE_THREADS, 0, s>>>(g.v, q.pen_par, q.started);
}

void queue_reset(hipStream_t s, const QueueGeom& g, const QueueBufs& q, uint32_t b, int num_cu) {
    if (b == 0) return;
    QueueResetArgs A{};
    A.state = g.state; A.started = q.started; A.ctl = q.ctl;
    A.layers = g.layers; A.num_batch = g.num_batch; A.b0 = g.b0; A.slot = g.slot;
    A.vec = g.slot % 4 == 0;
    A.slices = queue_slices(g, A.vec ? QUEUE_CHUNK : QUEUE_THREADS, num_cu);
    queue_reset_state_kernel<<<dim3(A.layers * A.slices, b), QUEUE_THREADS, 0, s>>>(A);
    queue_reset_occurrence(s, g, q, b);
}

void advance_queue_guided(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q,
                          uint32_t pairs) {
    if (q.seq_rows) advance_queue_guided_seq_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, pairs);
    else advance_queue_guided_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, pairs);
}

void queue_reset_guided(hipStream_t s, const QueueGeom& g, const QueueBufs& q, uint32_t pairs, int num_cu) {
    if (pairs == 0) return;
    QueueResetArgs A{};
    A.state = g.state; A.started = q.started; A.ctl = q.ctl;
    A.layers = g.layers; A.num_batch = g.num_batch; A.b0 = g.b0; A.slot = g.slot;
    A.vec = g.slot % 4 == 0;
    A.slices = queue_slices(g, A.vec ? QUEUE_CHUNK : QUEUE_THREADS, num_cu);
    queue_reset_state_guided_kernel<<<dim3(A.layers * A.slices, 2u * pairs), QUEUE_THREADS, 0, s>>>(A, pairs);
    // the occurrence rows are the pairs': reset where a pair takes a request, whenever its halves start
    QueueBufs rows = q;
    rows.started = q.pair_started;
    queue_reset_occurrence(s, g, rows, pairs);
}

void advance_queue_pool(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, const QueueBufs& q,
                        const QueueStateBufs& p, uint32_t b) {
    if (q.seq_rows) advance_queue_pool_seq_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, p, b);
    else advance_queue_pool_kernel<<<1, QUEUE_THREADS, 0, s>>>(drawn, tokens, history, counter, q, p, b);
}

void queue_turnover(hipStream_t s, const QueueGeom& g, const QueueBufs& q, const QueueStateBufs& p, uint32_t b, int num_cu) {
    if (b == 0) return;
    QueueTurnArgs A{};
    A.state = g.state; A.sctl = p.sctl; A.turn = p.turn; A.ctl = q.ctl;
    A.layers = g.layers; A.num_batch = g.num_batch; A.b0 = g.b0; A.slot = g.slot;
    A.slices = queue_slices(g, QUEUE_CHUNK, num_cu);
    queue_turnover_kernel<<<A.layers * A.slices, QUEUE_THREADS, 0, s>>>(A);
    if (p.history) queue_history_turnover(s, g.v, p.sctl, p.turn, q.pen_par, q.dry_par);
    else queue_reset_occurrence(s, g, q, b);
}

}  // namespace wrk

// ------------------------------------------------------------------ include/wrk_hip.h wrk_history_pool
static int32_t history_entry_check(wrk_ctx* ctx, const wrk_history_pool* hp, uint32_t k, const char* who) {
    WRK_ARG(ctx, !ctx->capturing_here(), "%s is blocking: not inside a capture", who);
    WRK_ARG(ctx, hp->ctx == ctx, "the history pool belongs to another context");
    WRK_ARG(ctx, k < hp->num_entries, "entry %u >= %u", k, hp->num_entries);
    return WRK_OK;
}

// wrk_history_pool_put / _get: slot `b` of `occ` and of `win` against entry k through queue_history_turnover on a list of one turn,
// the kernel of the queue's turnover.  The rules for the handles are those of a queue call with the pool
static int32_t history_move(wrk_ctx* ctx, wrk_history_pool* hp, uint32_t k, wrk_occurrence* occ, uint32_t b, wrk_token_window* win, bool put,
                            const char* who) {
    const int32_t rc = history_entry_check(ctx, hp, k, who);
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, occ || win, "an occurrence table or a token window is required");
    if (occ) {
        WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
        WRK_ARG(ctx, occ->num_vocab == hp->num_vocab, "occurrence table of %u tokens, history pool of %u", occ->num_vocab, hp->num_vocab);
        WRK_ARG(ctx, b < occ->num_batch, "slot %u >= %u", b, occ->num_batch);
    }
    WRK_ARG(ctx, win || hp->capacity == 0, "the history pool has windows: a token window is required");
    if (win) {
        WRK_ARG(ctx, win->ctx == ctx, "the token window belongs to another context");
        WRK_ARG(ctx, hp->capacity != 0, "the history pool was created without windows");
        WRK_ARG(ctx, win->capacity == hp->capacity, "token window of capacity %u, history pool of %u", win->capacity, hp->capacity);
        WRK_ARG(ctx, win->num_vocab == hp->num_vocab, "token window of %u tokens, history pool of %u", win->num_vocab, hp->num_vocab);
        WRK_ARG(ctx, b < win->num_batch, "slot %u >= %u", b, win->num_batch);
    }
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const wrk::QueueStateCtl sctl{nullptr, hp->num_entries, 1u, hp->dev()};
    const wrk::QueueTurn turn = put ? wrk::QueueTurn{0u, k, 0u, wrk::QUEUE_NO_ENTRY} : wrk::QueueTurn{0u, wrk::QUEUE_NO_ENTRY, 1u, k};
    wrk::PenaltyParam pen{};
    if (occ) pen = occ->row(b, 0.0f, 0.0f, 1.0f);
    wrk::DryParam dry{};
    if (win) { dry.ring = win->ring + (size_t)b * win->capacity; dry.meta = win->meta + (size_t)b * 2; dry.cap = win->capacity; }
    wrk_dev_arena dev;
    const size_t o_ctl = dev.add(sizeof sctl), o_turn = dev.add(sizeof turn), o_pen = dev.add(sizeof pen), o_dry = dev.add(sizeof dry);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_ctl), &sctl, sizeof sctl, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_turn), &turn, sizeof turn, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_pen), &pen, sizeof pen, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_dry), &dry, sizeof dry, hipMemcpyHostToDevice, ctx->stream));
    wrk::queue_history_turnover(ctx->stream, hp->num_vocab, dev.at<wrk::QueueStateCtl>(o_ctl), dev.at<wrk::QueueTurn>(o_turn),
                                occ ? dev.at<wrk::PenaltyParam>(o_pen) : nullptr, win ? dev.at<wrk::DryParam>(o_dry) : nullptr);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

extern "C" {

int32_t wrk_history_pool_create(wrk_ctx* ctx, uint32_t P, uint32_t V, uint32_t capacity, wrk_history_pool** out) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, P >= 1, "num_entries 0");
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, capacity <= WRK_MAX_TOKEN_WINDOW, "window_capacity %u: at most %u (0: no windows)", capacity, (uint32_t)WRK_MAX_TOKEN_WINDOW);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)P * V;
    wrk_dev_layout lay;
    const size_t o_c = lay.add(n * 4), o_f = lay.add(n), o_r = lay.add((size_t)P * capacity * 4), o_m = lay.add(capacity ? (size_t)P * 8 : 0);
    void* mem = nullptr;
    WRK_HIP(ctx, hipMalloc(&mem, lay.total));
    wrk_history_pool* hp = new wrk_history_pool;
    hp->ctx = ctx;
    hp->num_entries = P; hp->num_vocab = V; hp->capacity = capacity;
    hp->mem = mem;
    hp->counts = (float*)((char*)mem + o_c);
    hp->flags = (uint8_t*)((char*)mem + o_f);
    if (capacity) { hp->ring = (uint32_t*)((char*)mem + o_r); hp->meta = (uint32_t*)((char*)mem + o_m); }
    hipError_t e = hipMemsetAsync(mem, 0, lay.total, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        wrk_history_pool_destroy(hp);
        return wrk_fail(ctx, WRK_E_HIP, "history pool: %s", hipGetErrorString(e));
    }
    *out = hp;
    return WRK_OK;
}

int32_t wrk_history_pool_destroy(wrk_history_pool* hp) {
    if (!hp) return WRK_E_ARG;
    {
        std::lock_guard<std::recursive_mutex> lk(hp->ctx->mu);
        hipSetDevice(hp->ctx->device);
        hipStreamSynchronize(hp->ctx->stream);      // no step in flight still reads the pool
        hipFree(hp->mem);
    }
    delete hp;
    return WRK_OK;
}

int32_t wrk_history_pool_load(wrk_ctx* ctx, wrk_history_pool* hp, uint32_t k, const float* counts, const uint32_t* present,
                              const uint32_t* tokens, uint32_t n) {
    if (!ctx || !hp) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    int32_t rc = history_entry_check(ctx, hp, k, "wrk_history_pool_load");
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, (counts == nullptr) == (present == nullptr), "counts and present: both, or neither (an empty row)");
    const uint32_t V = hp->num_vocab, cap = hp->capacity;
    std::vector<float> c(V, 0.0f);
    std::vector<uint8_t> f(V, 0);
    for (uint32_t i = 0; counts && i < V; ++i) {
        WRK_ARG(ctx, finite_f32(counts[i]), "counts[%u] = %g: must be finite", i, (double)counts[i]);
        WRK_ARG(ctx, present[i] <= 1u, "present[%u] = %u: 0 or 1 (banned bits are not part of an entry)", i, present[i]);
        c[i] = counts[i];
        f[i] = (uint8_t)present[i];
    }
    if (!tokens) n = 0;
    WRK_ARG(ctx, n <= cap, "%u tokens, an entry's window holds %u", n, cap);
    for (uint32_t i = 0; i < n; ++i) WRK_ARG(ctx, tokens[i] < V, "token %u: id %u >= vocab %u", i, tokens[i], V);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    rc = wrk_buf_write_raw(ctx, hp->counts + (size_t)k * V, c.data(), (size_t)V * 4);
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, hp->flags + (size_t)k * V, f.data(), V);
    if (rc == WRK_OK && n) rc = wrk_buf_write_raw(ctx, hp->ring + (size_t)k * cap, tokens, (size_t)n * 4);
    const uint32_t meta[2] = {n, cap ? n % cap : 0u};
    if (rc == WRK_OK && cap) rc = wrk_buf_write_raw(ctx, hp->meta + (size_t)k * 2, meta, 8);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

int32_t wrk_history_pool_back(wrk_ctx* ctx, const wrk_history_pool* hp, uint32_t k, float* counts, uint32_t* present, uint32_t* tokens_out,
                              uint32_t* len) {
    if (!ctx || !hp) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const int32_t rc = history_entry_check(ctx, hp, k, "wrk_history_pool_back");
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, counts && present && len, "counts, present and len are required");
    const uint32_t V = hp->num_vocab, cap = hp->capacity;
    WRK_ARG(ctx, tokens_out || cap == 0, "tokens_out is required: the pool has windows");
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint8_t> f(V);
    std::vector<uint32_t> ring(cap);
    uint32_t meta[2] = {0u, 0u};
    WRK_HIP(ctx, hipMemcpyAsync(counts, hp->counts + (size_t)k * V, (size_t)V * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(f.data(), hp->flags + (size_t)k * V, V, hipMemcpyDeviceToHost, ctx->stream));
    if (cap) {
        WRK_HIP(ctx, hipMemcpyAsync(ring.data(), hp->ring + (size_t)k * cap, (size_t)cap * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(meta, hp->meta + (size_t)k * 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < V; ++i) present[i] = f[i];
    if (cap && (meta[0] > cap || meta[1] >= cap))
        return wrk_fail(ctx, WRK_E_HIP, "entry %u: inconsistent window (length %u position %u capacity %u)", k, meta[0], meta[1], cap);
    const uint32_t start = cap ? (meta[1] + cap - meta[0]) % cap : 0u;
    for (uint32_t j = 0; j < meta[0]; ++j) tokens_out[j] = ring[(start + j) % cap];
    *len = meta[0];
    return WRK_OK;
}

int32_t wrk_history_pool_put(wrk_ctx* ctx, wrk_history_pool* hp, uint32_t k, wrk_occurrence* occ, uint32_t b, wrk_token_window* win) {
    if (!ctx || !hp) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return history_move(ctx, hp, k, occ, b, win, true, "wrk_history_pool_put");
}

int32_t wrk_history_pool_get(wrk_ctx* ctx, wrk_history_pool* hp, uint32_t k, wrk_occurrence* occ, uint32_t b, wrk_token_window* win) {
    if (!ctx || !hp) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    return history_move(ctx, hp, k, occ, b, win, false, "wrk_history_pool_get");
}

}  // extern "C"
