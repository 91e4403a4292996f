// A request queue in the decode loops for gfx950.  R requests of different prompt and reply lengths are served on the
// B slots of a state inside one call: a slot whose request ends is reset and takes the next request in the same step program, so no
// slot waits for the longest reply of a batch.  A slot is a fixed-size recurrent state plus one "next token" word, so a refill is a
// fill of that state and another token in io.tokens; a prompt is taken in at decode rate by feeding its tokens in place of the draws.
//
//   advance_queue   takes advance_tokens' place in a queue program: one thread owns a slot, pops the next prompt token or takes the
//                   draw, checks the stop set and max_new, deals the next requests to the slots that ended (exclusive scan over the slot
//                   index from one next_request word), copies their parameters into the slot's rows, and moves the step counter last
//   queue_reset     grid (layer x slice, slot): every workgroup reads started[b] and leaves when it is 0; else zero fill / init_state
//                   copy of the slot, and a second small grid for the slot's occurrence row when the program is penalised
//   advance_queue_pool, queue_turnover   their places in the programs of a call with a state pool: the same advance body
//                   also lists the slots that ended; one (layer x slice) grid, whatever B, saves each listed slot's state to its
//                   request's pool entry and then fills the slot from the next request's entry, init_state or zeros
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

// slots are owned by the threads of ONE workgroup (B <= 256, as advance_stop).  POOL (advance_queue_pool_kernel): the slots that ended
// also go into the step's turnover list, at the position the scan below gives them.  SEQ (the _seq kernels): a reply draw
// goes through stop_seq_step (wrk_stopseq_dev.h) with the request's stop set and its StopSeqRow and enters the slot's tail; a match ends
// the request as a stop token does and leaves its match word; a slot that takes a request starts with an empty tail
template <bool POOL, bool SEQ>
__device__ __forceinline__ void advance_queue_body(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                   uint32_t* __restrict__ history, uint32_t* __restrict__ counter, const QueueBufs& Q,
                                                   const QueueStateBufs& P, uint32_t b) {
    __shared__ uint32_t wave_ended[QUEUE_WAVES];
    const uint32_t step = *counter;
    const uint32_t next = Q.ctl->next_request, live = Q.ctl->live, num_requests = Q.ctl->num_requests;
    const uint32_t i = threadIdx.x, lane = i & 63u, wave = i >> 6;
    int ended = 0;
    QueueSlot s{0u, 0u, 0u, QUEUE_IDLE};
    if (i < b) {
        s = Q.slots[i];
        const uint32_t y = drawn[i];
        history[(size_t)step * b + i] = y;     // a prompt-phase or idle draw too: the host cuts the replies out by the log
        if (s.phase == QUEUE_PROMPT) {
            const QueueReq* r = Q.reqs + s.req;
            s.pos += 1;
            tokens[i] = Q.pool[r->prompt_off + s.pos];
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
        uint32_t started = 0;
        QueueTurn turn{i, QUEUE_NO_ENTRY, 0u, QUEUE_NO_ENTRY};
        if (ended) {
            const uint32_t r = next + before + rank;
            if (POOL) turn.save = P.save[s.req];
            if (r < num_requests) {
                const QueueReq* q = Q.reqs + r;
                s = QueueSlot{r, 0u, 0u, q->prompt_len == 1 ? QUEUE_REPLY : QUEUE_PROMPT};
                tokens[i] = Q.pool[q->prompt_off];
                // reply token j is drawn at step (step + 1) + prompt_len - 1 + j: its sampler step is j whenever it is scheduled
                if (Q.sample_par) Q.sample_par[i] = SampleParam{q->temperature, q->top_p, q->seed, step + q->prompt_len};
                if (Q.filter_par) Q.filter_par[i] = SampleFilter{q->top_k, q->ln_min_p};
                // a refilled slot starts from its own request's mu, not from its predecessor's (a request is dispatched once: its entry
                // still holds its start value)
                if (Q.alt_par) Q.alt_par[i] = SampleAlt{q->tau, q->eta, Q.alt_mu ? Q.alt_mu[r] : 0.0f, q->typical_p};
                if (Q.gram_req) Q.gram_state[i] = Q.gram_req[r];        // the same for its automaton state
                // its DRY values and table, and an empty window: window_push, in front of this launch, has pushed the last draw of the
                // request that ended, and the next launch that reads the slot's window is the next step's dry_rows
                if (Q.dry_par) {
                    DryParam* dp = Q.dry_par + i;
                    const DryParam* dq = Q.dry_req + r;
                    dp->allowed = dq->allowed; dp->no_repeat = dq->no_repeat; dp->multiplier = dq->multiplier;
                    for (uint32_t m = 0; m <= WRK_DRY_MAX_MATCH; ++m) dp->pen[m] = dq->pen[m];
                    dp->meta[0] = 0u; dp->meta[1] = 0u;
                }
                if (SEQ) stop_tail_clear(Q.seq_tail + (size_t)i * STOP_TAIL);      // and its tail starts empty
                if (Q.pen_par) { Q.pen_par[i].presence = q->presence; Q.pen_par[i].frequency = q->frequency; Q.pen_par[i].decay = q->decay; }
                Q.log[r] = QueueLog{0u, 3u, i, step + 1};
                started = 1;
                if (POOL) { turn.started = 1; turn.start = P.start[r]; }
            } else {
                s.phase = QUEUE_IDLE;
            }
            if (POOL) P.turn[before + rank] = turn;
        }
        Q.slots[i] = s;
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

struct QueueResetArgs {
    float* state;               // [L][num_batch][slot] f32
    const uint32_t* started;
    const QueueCtl* ctl;
    uint32_t layers, slices, num_batch, b0, vec;
    size_t slot;                // (S + 2) * D
};

__global__ void __launch_bounds__(QUEUE_THREADS) queue_reset_state_kernel(const QueueResetArgs A) {
    const uint32_t b = blockIdx.y;
    if (A.started[b] == 0) return;
    const uint32_t l = blockIdx.x / A.slices, part = blockIdx.x - l * A.slices;
    float* dst = A.state + ((size_t)l * A.num_batch + A.b0 + b) * A.slot;
    const float* init = A.ctl->init_state;
    const float* src = init ? init + (size_t)l * A.slot : nullptr;
    const size_t n = A.slot;
    if (A.vec && (((uintptr_t)src) & 15u) == 0) {
        for (size_t i = (size_t)part * QUEUE_CHUNK + threadIdx.x * 4; i < n; i += (size_t)A.slices * QUEUE_CHUNK)
            *(f32x4*)(dst + i) = src ? *(const f32x4*)(src + i) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
        for (size_t i = (size_t)part * QUEUE_THREADS + threadIdx.x; i < n; i += (size_t)A.slices * QUEUE_THREADS) dst[i] = src ? src[i] : 0.0f;
    }
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
    queue_reset_occurrence(s, g, q, b);
}

}  // namespace wrk
