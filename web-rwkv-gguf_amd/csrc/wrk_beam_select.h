// Beam search's pure rule (include/wrk_hip.h wrk_v7_generate_beam), free of HIP: what a candidate is, the order of a
// group's candidates, and the placement of the survivors with the status every slot then has.  beam_select_kernel (wrk_beam.hip) finds
// the order with one wave per group and runs beam_place on the device; beam_select_group is the whole rule on one thread, which the
// host test runs over this header alone.  wrk_internal.h includes it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wrk_hip.h"

#ifndef WRK_HD
#ifdef __HIPCC__
#define WRK_HD __host__ __device__
#else
#define WRK_HD
#endif
#endif

namespace wrk {

// a slot's record: score = the f32 sum of its log-probs, key = what it is ordered by (raw * inv_norm[len] when it was placed; the
// start slot: 0; a DEAD slot: -inf), length = generated tokens, status = WRK_BEAM_LIVE / _DONE / _DEAD
struct BeamSlot { float score, key; uint32_t length, status; };
// a group's stop set, ids ascending (the host sorts them)
struct BeamStop { uint32_t count; uint32_t ids[WRK_MAX_BEAM_STOP_TOKENS]; };
// a candidate of a group.  origin: the slot within the group it comes from; j: its rank in that slot's row (0 for a DONE slot);
// token: what the slot it is placed in feeds next, WRK_BEAM_NO_TOKEN for a DONE slot, which stays where it is
struct BeamCand { float key, raw; uint32_t origin, j, len, token; };

static constexpr uint32_t BEAM_MAX_CANDS = WRK_MAX_BEAMS * WRK_MAX_BEAMS + WRK_MAX_BEAMS;

// a token whose log-prob is -inf or NaN is no candidate
WRK_HD inline bool beam_lp_ok(float lp) { return lp == lp && lp != -__builtin_inff(); }

// candidate (origin, j) of a LIVE slot: one f32 addition, one f32 multiplication with the host's table
WRK_HD inline BeamCand beam_live_cand(const BeamSlot& s, uint32_t origin, uint32_t j, uint32_t token, float lp, const float* inv_norm) {
    const float raw = s.score + lp;
    const uint32_t len = s.length + 1;
    const float key = raw * inv_norm[len];
    return BeamCand{key, raw, origin, j, len, token};
}

// a DONE slot's one candidate: itself, with the key it got when it ended
WRK_HD inline BeamCand beam_done_cand(const BeamSlot& s, uint32_t origin) {
    return BeamCand{s.key, s.score, origin, 0u, s.length, WRK_BEAM_NO_TOKEN};
}

// whether `token` is in the stop set: a binary search of the sorted ids
WRK_HD inline bool beam_is_stop(const BeamStop& stop, uint32_t token) {
    uint32_t lo = 0, hi = stop.count < WRK_MAX_BEAM_STOP_TOKENS ? stop.count : WRK_MAX_BEAM_STOP_TOKENS;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (stop.ids[mid] < token) lo = mid + 1; else hi = mid;
    }
    return lo < stop.count && lo < WRK_MAX_BEAM_STOP_TOKENS && stop.ids[lo] == token;
}

// THE order: key descending, ties by slot of origin ascending, then j ascending
WRK_HD inline bool beam_before(const BeamCand& a, const BeamCand& b) {
    if (a.key != b.key) return a.key > b.key;
    if (a.origin != b.origin) return a.origin < b.origin;
    return a.j < b.j;
}

// THE placement: sv[0 .. n) are the survivors in order (n <= w).  A surviving DONE slot keeps its place and its record; the group's
// other slots, ascending, take the live survivors in their order, DONE when the token is in the stop set; the rest become DEAD.
// Per slot of the group: its record, the token it feeds next (NO_TOKEN: not filled in this step), its parent (a slot of the group;
// itself when not filled) and whether it ended in this step.  `in` and `out` do not overlap
WRK_HD inline void beam_place(const BeamSlot* in, const BeamCand* sv, uint32_t n, uint32_t w, const BeamStop& stop, BeamSlot* out, uint32_t* token,
                              uint32_t* parent, uint32_t* ended) {
    bool taken[WRK_MAX_BEAMS];
    for (uint32_t q = 0; q < w; ++q) {
        out[q] = BeamSlot{-__builtin_inff(), -__builtin_inff(), 0u, (uint32_t)WRK_BEAM_DEAD};
        token[q] = WRK_BEAM_NO_TOKEN; parent[q] = q; ended[q] = 0u; taken[q] = false;
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (sv[i].token != WRK_BEAM_NO_TOKEN) continue;
        const uint32_t q = sv[i].origin;
        out[q] = in[q];
        taken[q] = true;
    }
    uint32_t q = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (sv[i].token == WRK_BEAM_NO_TOKEN) continue;
        while (q < w && taken[q]) ++q;
        if (q >= w) break;              // never: at most w survivors
        const bool is_stop = beam_is_stop(stop, sv[i].token);
        out[q] = BeamSlot{sv[i].raw, sv[i].key, sv[i].len, (uint32_t)(is_stop ? WRK_BEAM_DONE : WRK_BEAM_LIVE)};
        token[q] = sv[i].token; parent[q] = sv[i].origin; ended[q] = is_stop ? 1u : 0u;
        taken[q] = true;
    }
}

// One group's step on one thread: in[w] the records; ids / lp [w][w]: row b's w first tokens in the sampler's order and their
// log-probs (only read for LIVE slots); outputs as beam_place
WRK_HD inline void beam_select_group(const BeamSlot* in, uint32_t w, const uint32_t* ids, const float* lp, const float* inv_norm, const BeamStop& stop,
                                     BeamSlot* out, uint32_t* token, uint32_t* parent, uint32_t* ended) {
    BeamCand c[BEAM_MAX_CANDS];
    bool used[BEAM_MAX_CANDS];
    uint32_t nc = 0;
    for (uint32_t b = 0; b < w; ++b) {
        if (in[b].status == WRK_BEAM_DONE) c[nc++] = beam_done_cand(in[b], b);
        if (in[b].status != WRK_BEAM_LIVE) continue;
        for (uint32_t j = 0; j < w; ++j)
            if (beam_lp_ok(lp[b * w + j])) c[nc++] = beam_live_cand(in[b], b, j, ids[b * w + j], lp[b * w + j], inv_norm);
    }
    for (uint32_t i = 0; i < nc; ++i) used[i] = false;
    BeamCand sv[WRK_MAX_BEAMS];
    uint32_t n = 0;
    while (n < w && n < nc) {
        uint32_t best = BEAM_MAX_CANDS;
        for (uint32_t i = 0; i < nc; ++i)
            if (!used[i] && (best == BEAM_MAX_CANDS || beam_before(c[i], c[best]))) best = i;
        used[best] = true;
        sv[n++] = c[best];
    }
    beam_place(in, sv, n, w, stop, out, token, parent, ended);
}

}  // namespace wrk
