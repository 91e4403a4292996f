// The stop-sequence matcher of the decode loops: one owner's counted draw.  It exists once, here, for the three kernels
// that run it -- advance_stop_seq_kernel (wrk_stop.hip), the queue's advance kernels (wrk_queue.hip) and stop_seq_rows_kernel
// (wrk_stop.hip, behind wrk_stop_sequences_advance) -- so that a stop program, a queue program and a host-driven loop end a reply at the
// same draw with the same match word.
//
// An owner's tail is its last WRK_STOP_TAIL_LEN counted draws, oldest first, right aligned, WRK_STOP_TAIL_EMPTY where there is none yet.
// A stop sequence of length l matches at the draw y when the last l entries of (tail ++ [y]) equal it.  The rows hold every sequence
// reversed, so entry 0 is compared with y and entry j with tail[LEN - j]: the usual step costs one compare per sequence, and EMPTY, which
// equals no id, makes a sequence that would reach across the start of the tail fail without a length test.  One thread does the whole
// owner: the 8 x 8 worst case is 64 compares on 7 tail registers (every tail index below is a compile-time constant: no scratch).
// Plain loads and stores only; no atomics; nothing waits.
#pragma once
#include "wrk_device.h"
#include "wrk_internal.h"

namespace wrk {

static constexpr uint32_t STOP_TAIL = WRK_STOP_TAIL_LEN;
static_assert(WRK_MAX_STOP_SEQUENCE_LEN == WRK_STOP_TAIL_LEN + 1, "a sequence is matched against the tail and the drawn token");

// the tail words of one owner in registers
struct StopTail { uint32_t t[STOP_TAIL]; };

__device__ __forceinline__ StopTail stop_tail_load(const uint32_t* __restrict__ p) {
    StopTail a;
#pragma unroll
    for (uint32_t j = 0; j < STOP_TAIL; ++j) a.t[j] = p[j];
    return a;
}

__device__ __forceinline__ void stop_tail_store(uint32_t* __restrict__ p, const StopTail& a) {
#pragma unroll
    for (uint32_t j = 0; j < STOP_TAIL; ++j) p[j] = a.t[j];
}

// The counted draw y of one owner: the match word -- WRK_STOP_MATCH_NONE, WRK_STOP_MATCH_TOKEN (y is one of ids[0 .. nids)) or the index
// of the matching sequence of `row`; the longest match wins, at equal length the stop-set id beats a sequence and the lower index the
// higher -- and the tail moved on by y, match or not (the draw that ends an owner counts).  row == nullptr: no sequences
__device__ __forceinline__ uint32_t stop_seq_step(StopTail& tail, uint32_t y, const StopSeqRow* __restrict__ row, const uint32_t* __restrict__ ids,
                                                  uint32_t nids) {
    uint32_t match = WRK_STOP_MATCH_NONE, best = 0;
    const uint32_t n = nids < WRK_MAX_STOP_TOKENS ? nids : WRK_MAX_STOP_TOKENS;
    int hit = 0;
    for (uint32_t k = 0; k < n; ++k) hit |= (ids[k] == y);
    if (hit) { match = WRK_STOP_MATCH_TOKEN; best = 1; }
    // every sequence's last id and length are fetched before any is looked at: eight independent loads in flight, one memory latency
    // for the usual step, where a loop that leaves at the first mismatch would pay one per sequence.  A row is a whole StopSeqRow
    // whatever its count, so the loads stay inside it
    uint32_t ns = 0, last[WRK_MAX_STOP_SEQUENCES] = {}, len[WRK_MAX_STOP_SEQUENCES] = {};
    if (row) {
        ns = row->count < WRK_MAX_STOP_SEQUENCES ? row->count : WRK_MAX_STOP_SEQUENCES;
#pragma unroll
        for (uint32_t k = 0; k < WRK_MAX_STOP_SEQUENCES; ++k) { last[k] = row->tok[k][0]; len[k] = row->len[k]; }
    }
#pragma unroll
    for (uint32_t k = 0; k < WRK_MAX_STOP_SEQUENCES; ++k) {
        if (k >= ns || last[k] != y) continue;  // the usual step ends here
        const uint32_t l = len[k];
        if (l <= best || l > WRK_MAX_STOP_SEQUENCE_LEN) continue;      // a longer or an earlier match stands (the host validates 1 <= l <= 8)
        const uint32_t* __restrict__ q = row->tok[k];
        int ok = 1;
#pragma unroll
        for (uint32_t j = 1; j < WRK_MAX_STOP_SEQUENCE_LEN; ++j)
            if (j < l) ok &= (q[j] == tail.t[STOP_TAIL - j]);
        if (ok) { match = k; best = l; }
    }
#pragma unroll
    for (uint32_t j = 0; j + 1 < STOP_TAIL; ++j) tail.t[j] = tail.t[j + 1];
    tail.t[STOP_TAIL - 1] = y;
    return match;
}

}  // namespace wrk
