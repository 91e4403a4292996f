// Stop tokens in the decode loops for gfx950.  A sequence ends at the step that draws one of its stop ids; it keeps
// running through the layers (no model kernel knows about it), and the step that ends it snapshots its state slot and its logits row
// on the device.  After the loop the snapshot is put back, so the slot holds the state after the tokens before the stop token.
//
//   advance_stop    takes advance_tokens' place in a stop program: one thread owns a sequence, reads its StopParam row, writes
//                   history / tokens, marks a sequence that has just drawn a stop id, and moves the step counter last
//   stop_snapshot   grid (layer x slice + logits slices, sequence): every workgroup reads just_ended[b] and leaves when it is 0
//   stop_restore    once after the loop, outside the captured program: snapshot -> state and logits of the sequences that are done
//   advance_stop_seq   advance_stop's place in a stop program with stop sequences: the same, and the sequence's draw also
//                   goes through the matcher of wrk_stopseq_dev.h, which moves its tail and, where it ends, leaves its match word
//   stop_seq_rows   the matcher alone on n rows, behind wrk_stop_sequences_advance
//
// just_ended[b] is written by EVERY advance_stop launch for every sequence (1 when the sequence ended in this step, else 0), so the flag
// a snapshot launch reads was written by the advance_stop launch in front of it in the same stream; nothing has to clear it.
// Plain vector stores only; no atomics; no kernel waits on another.
#include "wrk_device.h"
#include "wrk_runner.h"
#include "wrk_stopseq_dev.h"

namespace wrk {

static constexpr uint32_t STOP_THREADS = 256;
static constexpr uint32_t STOP_CHUNK = STOP_THREADS * 4;       // floats a workgroup moves per pass (16 bytes per thread)

// sequences are owned by the threads of ONE workgroup (B <= 256, as advance_tokens)
__global__ void __launch_bounds__(STOP_THREADS) advance_stop_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                    uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                    StopParam* __restrict__ par, uint32_t* __restrict__ just_ended,
                                                                    uint32_t* __restrict__ live, uint32_t b) {
    const uint32_t step = *counter;
    const uint32_t i = threadIdx.x;
    int ended = 0;
    if (i < b) {
        StopParam* p = par + i;
        if (p->done) {
            history[(size_t)step * b + i] = p->end_token;      // tokens[i] stays: a valid id keeps flowing through the embedding gather
        } else {
            const uint32_t y = drawn[i];
            tokens[i] = y;
            history[(size_t)step * b + i] = y;
            const uint32_t n = p->count < WRK_MAX_STOP_TOKENS ? p->count : WRK_MAX_STOP_TOKENS;
            for (uint32_t k = 0; k < n; ++k) ended |= (p->ids[k] == y);
            if (ended) { p->done = 1; p->length = step + 1; p->end_token = y; }
        }
        just_ended[i] = (uint32_t)ended;
    }
    const int n_ended = __syncthreads_count(ended);     // also orders every read of *counter before its update
    if (i == 0) {
        if (n_ended) *live = *live - (uint32_t)n_ended;
        *counter = step + 1;
    }
}

// advance_stop_kernel for stop programs with stop sequences: the same workgroup, ownership and ordering.  The draw of a
// sequence that is still running goes through stop_seq_step (wrk_stopseq_dev.h) with its stop set and its StopSeqRow; the tail takes it
// in, and the step that ends the sequence also writes its match word.  A finished sequence's tail and match word are never touched again
__global__ void __launch_bounds__(STOP_THREADS) advance_stop_seq_kernel(const uint32_t* __restrict__ drawn, uint32_t* __restrict__ tokens,
                                                                        uint32_t* __restrict__ history, uint32_t* __restrict__ counter,
                                                                        StopParam* __restrict__ par, uint32_t* __restrict__ just_ended,
                                                                        uint32_t* __restrict__ live, const StopSeqBufs Q, uint32_t b) {
    const uint32_t step = *counter;
    const uint32_t i = threadIdx.x;
    int ended = 0;
    if (i < b) {
        StopParam* p = par + i;
        if (p->done) {
            history[(size_t)step * b + i] = p->end_token;
        } else {
            const uint32_t y = drawn[i];
            tokens[i] = y;
            history[(size_t)step * b + i] = y;
            uint32_t* tp = Q.tail + (size_t)i * STOP_TAIL;
            StopTail tail = stop_tail_load(tp);
            const uint32_t match = stop_seq_step(tail, y, Q.rows + i, p->ids, p->count);
            stop_tail_store(tp, tail);
            ended = match != WRK_STOP_MATCH_NONE;
            if (ended) { p->done = 1; p->length = step + 1; p->end_token = y; Q.match[i] = match; }
        }
        just_ended[i] = (uint32_t)ended;
    }
    const int n_ended = __syncthreads_count(ended);     // also orders every read of *counter before its update
    if (i == 0) {
        if (n_ended) *live = *live - (uint32_t)n_ended;
        *counter = step + 1;
    }
}

// wrk_stop_sequences_advance: one owner per thread, any number of rows
__global__ void __launch_bounds__(STOP_THREADS) stop_seq_rows_kernel(uint32_t n, const StopSeqRow* __restrict__ rows, const StopParam* __restrict__ ids,
                                                                     uint32_t* __restrict__ tail, const uint32_t* __restrict__ tokens,
                                                                     uint32_t* __restrict__ match) {
    const uint32_t r = blockIdx.x * STOP_THREADS + threadIdx.x;
    if (r >= n) return;
    uint32_t* tp = tail + (size_t)r * STOP_TAIL;
    StopTail t = stop_tail_load(tp);
    match[r] = stop_seq_step(t, tokens[r], rows + r, ids ? ids[r].ids : nullptr, ids ? ids[r].count : 0u);
    stop_tail_store(tp, t);
}

// 16-byte copies of n floats (n % 4 == 0, both 16-byte aligned), or scalar ones; workgroup `part` of `parts`
__device__ __forceinline__ void stop_copy(const float* __restrict__ src, float* __restrict__ dst, size_t n, bool vec, uint32_t part,
                                          uint32_t parts) {
    if (vec) {
        for (size_t i = (size_t)part * STOP_CHUNK + threadIdx.x * 4; i < n; i += (size_t)parts * STOP_CHUNK)
            *(f32x4*)(dst + i) = *(const f32x4*)(src + i);
    } else {
        for (size_t i = (size_t)part * STOP_THREADS + threadIdx.x; i < n; i += (size_t)parts * STOP_THREADS) dst[i] = src[i];
    }
}

// RESTORE = false: state slot / head_o row -> snapshot of the sequences with just_ended[b];  true: snapshot -> state slot / head_o row
// of the sequences with par[b].done.  blockIdx.x < layers * slices: slice of one layer's slot; above: slice of the logits row.
struct StopCopyArgs {
    float* state;               // [L][num_batch][slot] f32
    float* head_o;              // [B][V]
    float* snap_state;          // [B][L][slot]
    float* snap_logits;         // [B][V]
    const uint32_t* just_ended;
    const StopParam* par;
    const uint32_t* counter;    // restore: lengths of sequences that never ended
    uint32_t* lengths;          // restore: [B]
    uint32_t layers, slices, lslices, num_batch, b0, v, vec_state, vec_logits;
    size_t slot;                // (S + 2) * D
};

template <bool RESTORE>
__global__ void __launch_bounds__(STOP_THREADS) stop_copy_kernel(const StopCopyArgs A) {
    const uint32_t b = blockIdx.y;
    const bool on = RESTORE ? A.par[b].done != 0 : A.just_ended[b] != 0;
    if (RESTORE && blockIdx.x == 0 && threadIdx.x == 0) A.lengths[b] = on ? A.par[b].length : *A.counter;
    if (!on) return;
    const uint32_t x = blockIdx.x;
    if (x < A.layers * A.slices) {
        const uint32_t l = x / A.slices, part = x - l * A.slices;
        float* live_slot = A.state + ((size_t)l * A.num_batch + A.b0 + b) * A.slot;
        float* snap = A.snap_state + ((size_t)b * A.layers + l) * A.slot;
        if (RESTORE) stop_copy(snap, live_slot, A.slot, A.vec_state != 0, part, A.slices);
        else stop_copy(live_slot, snap, A.slot, A.vec_state != 0, part, A.slices);
    } else {
        const uint32_t part = x - A.layers * A.slices;
        float* row = A.head_o + (size_t)b * A.v;
        float* snap = A.snap_logits + (size_t)b * A.v;
        if (RESTORE) stop_copy(snap, row, A.v, A.vec_logits != 0, part, A.lslices);
        else stop_copy(row, snap, A.v, A.vec_logits != 0, part, A.lslices);
    }
}

void advance_stop(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, StopParam* par,
                  uint32_t* just_ended, uint32_t* live, uint32_t b) {
    advance_stop_kernel<<<1, STOP_THREADS, 0, s>>>(drawn, tokens, history, counter, par, just_ended, live, b);
}

void advance_stop_seq(hipStream_t s, const uint32_t* drawn, uint32_t* tokens, uint32_t* history, uint32_t* counter, StopParam* par,
                      uint32_t* just_ended, uint32_t* live, const StopSeqBufs& q, uint32_t b) {
    advance_stop_seq_kernel<<<1, STOP_THREADS, 0, s>>>(drawn, tokens, history, counter, par, just_ended, live, q, b);
}

void stop_seq_rows(hipStream_t s, uint32_t n, const StopSeqRow* rows, const StopParam* ids, uint32_t* tail, const uint32_t* tokens, uint32_t* match) {
    if (n == 0) return;
    stop_seq_rows_kernel<<<(n + STOP_THREADS - 1) / STOP_THREADS, STOP_THREADS, 0, s>>>(n, rows, ids, tail, tokens, match);
}

// slices of a layer's slot: layers * slices workgroups come to about two per CU, so that one ending sequence's copy (13 MB at the
// 1.5B shape) runs on the whole chip, and no slice is smaller than one pass
static StopCopyArgs stop_copy_args(const StopGeom& g, int num_cu) {
    StopCopyArgs A{};
    A.state = g.state; A.head_o = g.head_o; A.snap_state = g.snap_state; A.snap_logits = g.snap_logits;
    A.just_ended = g.just_ended; A.par = g.par; A.counter = g.counter; A.lengths = g.lengths;
    A.layers = g.layers; A.num_batch = g.num_batch; A.b0 = g.b0; A.v = g.v; A.slot = g.slot;
    A.vec_state = g.slot % 4 == 0;
    A.vec_logits = g.v % 4 == 0;
    const uint32_t per_pass = A.vec_state ? STOP_CHUNK : STOP_THREADS;
    const uint32_t max_slices = (uint32_t)((g.slot + per_pass - 1) / per_pass);
    uint32_t want = (2u * (uint32_t)num_cu + g.layers - 1) / g.layers;
    A.slices = want < 1 ? 1 : (want > max_slices ? max_slices : want);
    const uint32_t lpass = A.vec_logits ? STOP_CHUNK : STOP_THREADS;
    const uint32_t lmax = (g.v + lpass - 1) / lpass;
    A.lslices = lmax < 16 ? lmax : 16;
    return A;
}

void stop_snapshot(hipStream_t s, const StopGeom& g, uint32_t b, int num_cu) {
    if (b == 0) return;
    const StopCopyArgs A = stop_copy_args(g, num_cu);
    stop_copy_kernel<false><<<dim3(A.layers * A.slices + A.lslices, b), STOP_THREADS, 0, s>>>(A);
}

void stop_restore(hipStream_t s, const StopGeom& g, uint32_t b, int num_cu) {
    if (b == 0) return;
    const StopCopyArgs A = stop_copy_args(g, num_cu);
    stop_copy_kernel<true><<<dim3(A.layers * A.slices + A.lslices, b), STOP_THREADS, 0, s>>>(A);
}

}  // namespace wrk
