// Beam search in the decode loops for gfx950 (the rule: wrk_beam_select.h).
//
//   beam_step_rows   the candidate front -- logprob_rows (wrk_logprob.hip) with num_top = W, so a row's candidates are wrk_top_logprobs'
//                    bits -- and beam_select
//   beam_select      one workgroup of four waves, a wave per group (groups beyond four in turn).  Lane o < W owns slot o of the group:
//                    a LIVE slot's candidates are sorted already -- raw = score + lp and key = raw * inv_norm are monotone in lp and ties
//                    go by j ascending -- and a DONE slot has one, so the group's order is a merge of at most W sorted lists: W rounds of
//                    "the best head", a wave butterfly over (key, origin) under beam_before.  Lane 0 then runs beam_place on the
//                    survivors, and lanes < W write their slot: the record, the token it feeds next, the history row, the copy list
//                    and the snapshot / done maps.  Thread 0 writes the LIVE count and moves the step counter last
//   beam_copy        grid (layer x slice, slot): dst slot q <- src slot (map[q] or q) for every listed q over all layers, cut over
//                    about two workgroups per CU as stop_snapshot is; workgroups of the other slots return at once
//   beam_permute     state slot q <- state slot map[q] under any aliasing: two beam_copy launches through a scratch.  The gather only
//                    reads the state and only writes the scratch, the scatter only reads the scratch and only writes the state, and the
//                    stream orders the two: no slot is written before every slot has been read
//   beam_context     grid (slice, slot): the same gather and scatter for what a hypothesis carries beside its state -- its
//                    occurrence row, token window and automaton state -- through a scratch of context rows.  Slice x moves elements
//                    [1024 x, 1024 (x + 1)) of the counts, the flags and the ring; slice 0's first thread also the meta and state words
// Plain vector stores only; no atomics; no kernel waits on another.
#include "wrk_rows_dev.h"
#include "wrk_runner.h"

#include <algorithm>

namespace wrk {

static constexpr uint32_t BEAM_THREADS = 256;
static constexpr uint32_t BEAM_WAVES = BEAM_THREADS / WAVE;
static constexpr uint32_t BEAM_CHUNK = BEAM_THREADS * 4;       // floats a workgroup moves per pass (16 bytes per thread)
static constexpr uint32_t BEAM_NO_LANE = 64;

__global__ void __launch_bounds__(BEAM_THREADS) beam_select_kernel(const BeamBufs Q, uint32_t* __restrict__ tokens, uint32_t* __restrict__ counter,
                                                                   uint32_t b) {
    __shared__ BeamSlot sm_in[BEAM_WAVES][WRK_MAX_BEAMS], sm_out[BEAM_WAVES][WRK_MAX_BEAMS];
    __shared__ BeamCand sm_sv[BEAM_WAVES][WRK_MAX_BEAMS];
    __shared__ uint32_t sm_tok[BEAM_WAVES][WRK_MAX_BEAMS], sm_par[BEAM_WAVES][WRK_MAX_BEAMS], sm_end[BEAM_WAVES][WRK_MAX_BEAMS];
    __shared__ uint32_t sm_live[BEAM_WAVES];
    const uint32_t step = *counter;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t w = Q.par->w < WRK_MAX_BEAMS ? Q.par->w : WRK_MAX_BEAMS;
    const uint32_t groups = w ? b / w : 0u;
    // a step past the history rows or the inv_norm table selects nothing (the host never submits one)
    const bool room = step < Q.par->hist_rows && step + 1 < Q.par->inv_len;
    uint32_t live = 0;
    for (uint32_t g0 = 0; room && g0 < groups; g0 += BEAM_WAVES) {
        const uint32_t g = g0 + wid;
        const bool active = g < groups;
        const bool mine = active && lane < w;
        BeamSlot me{0.0f, 0.0f, 0u, (uint32_t)WRK_BEAM_DEAD};
        if (mine) { me = Q.slots[g * w + lane]; sm_in[wid][lane] = me; }
        const bool is_live = mine && me.status == WRK_BEAM_LIVE, is_done = mine && me.status == WRK_BEAM_DONE;
        const size_t row = (size_t)(g * w + lane) * w;
        uint32_t h = 0, n = 0;          // h: the head of this lane's list
        for (uint32_t r = 0; r < w; ++r) {
            BeamCand c{0.0f, 0.0f, lane, 0u, 0u, 0u};
            bool has = false;
            if (is_live) {
                while (h < w && !beam_lp_ok(Q.cand_lp[row + h])) ++h;
                if (h < w) { c = beam_live_cand(me, lane, h, Q.cand_ids[row + h], Q.cand_lp[row + h], Q.inv_norm); has = true; }
            } else if (is_done && h == 0) {
                c = beam_done_cand(me, lane);
                has = true;
            }
            // heads come from different slots: (key, origin) decides between two of them
            uint32_t best_lane = has ? lane : BEAM_NO_LANE;
            float best_key = c.key;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t ol = __shfl_xor(best_lane, o, WAVE);
                const float ok = __shfl_xor(best_key, o, WAVE);
                const BeamCand mine_c{best_key, 0.0f, best_lane, 0u, 0u, 0u}, other_c{ok, 0.0f, ol, 0u, 0u, 0u};
                if (ol != BEAM_NO_LANE && (best_lane == BEAM_NO_LANE || beam_before(other_c, mine_c))) { best_lane = ol; best_key = ok; }
            }
            if (best_lane == BEAM_NO_LANE) break;       // uniform: the group has no candidate left
            if (lane == best_lane) { sm_sv[wid][r] = c; ++h; }
            ++n;
        }
        __syncthreads();
        if (active && lane == 0) beam_place(sm_in[wid], sm_sv[wid], n, w, Q.stops[g], sm_out[wid], sm_tok[wid], sm_par[wid], sm_end[wid]);
        __syncthreads();
        bool now_live = false;
        if (mine) {
            const uint32_t q = g * w + lane;
            const BeamSlot o = sm_out[wid][lane];
            const uint32_t t = sm_tok[wid][lane], p = sm_par[wid][lane];
            Q.slots[q] = o;
            if (t != WRK_BEAM_NO_TOKEN) tokens[q] = t;      // every other slot goes on feeding the valid id it holds
            const size_t at = (size_t)step * b + q;
            Q.step_tokens[at] = t;
            Q.step_parents[at] = g * w + p;
            Q.step_scores[at] = o.score;
            Q.copy_src[q] = (t != WRK_BEAM_NO_TOKEN && p != lane) ? g * w + p : WRK_BEAM_NO_COPY;
            Q.snap_map[q] = sm_end[wid][lane] ? q : WRK_BEAM_NO_COPY;
            Q.done_map[q] = o.status == WRK_BEAM_DONE ? q : WRK_BEAM_NO_COPY;
            Q.filled[q] = t != WRK_BEAM_NO_TOKEN ? 1u : 0u;
            now_live = o.status == WRK_BEAM_LIVE;
        }
        live += (uint32_t)__popcll(__ballot(now_live));
    }
    if (lane == 0) sm_live[wid] = live;
    __syncthreads();        // also orders every read of *counter before its update
    if (tid == 0) {
        if (room) {
            uint32_t total = 0;
            for (uint32_t k = 0; k < BEAM_WAVES; ++k) total += sm_live[k];
            *Q.live = total;
        }
        *counter = step + 1;
    }
}

struct BeamCopyArgs {
    const float* src; float* dst;
    uint32_t src_nb, src_b0, dst_nb, dst_b0;
    const uint32_t* map;
    uint32_t src_mapped, layers, slices, vec;
    size_t slot;
};

__global__ void __launch_bounds__(BEAM_THREADS) beam_copy_kernel(const BeamCopyArgs A) {
    const uint32_t q = blockIdx.y;
    const uint32_t m = A.map[q];
    if (m == WRK_BEAM_NO_COPY) return;
    const uint32_t l = blockIdx.x / A.slices, part = blockIdx.x - l * A.slices;
    const float* __restrict__ src = A.src + ((size_t)l * A.src_nb + A.src_b0 + (A.src_mapped ? m : q)) * A.slot;
    float* __restrict__ dst = A.dst + ((size_t)l * A.dst_nb + A.dst_b0 + q) * A.slot;
    if (A.vec) {
        for (size_t i = (size_t)part * BEAM_CHUNK + threadIdx.x * 4; i < A.slot; i += (size_t)A.slices * BEAM_CHUNK)
            *(f32x4*)(dst + i) = *(const f32x4*)(src + i);
    } else {
        for (size_t i = (size_t)part * BEAM_THREADS + threadIdx.x; i < A.slot; i += (size_t)A.slices * BEAM_THREADS) dst[i] = src[i];
    }
}

// one direction of the context permutation: SCATTER false -- scratch row q <- slot map[q]; true -- slot q <- scratch row q
struct BeamCtxArgs {
    BeamCtxRows rows; BeamCtxScratch tmp;
    const uint32_t* map;
    uint32_t v;
};

template <bool VEC, bool SCATTER>
__global__ void __launch_bounds__(BEAM_THREADS) beam_context_kernel(const BeamCtxArgs A) {
    const uint32_t q = blockIdx.y;
    const uint32_t m = A.map[q];
    if (m == WRK_BEAM_NO_COPY) return;
    const uint32_t tid = threadIdx.x, base = blockIdx.x * BEAM_CHUNK, v = A.v;
    const uint32_t slot = SCATTER ? q : m;      // the table's side of the move; the scratch's side is row q
    if (A.rows.pen && base < v) {
        const PenaltyParam p = A.rows.pen[slot];
        float* tc = A.tmp.count + (size_t)q * v;
        uint8_t* tf = A.tmp.flags + (size_t)q * v;
        if (VEC) {
            const uint32_t i = base + tid * 4;
            if (i < v) {
                if (SCATTER) { *(f32x4*)(p.count + i) = *(const f32x4*)(tc + i); *(uint32_t*)(p.flags + i) = *(const uint32_t*)(tf + i); }
                else { *(f32x4*)(tc + i) = *(const f32x4*)(p.count + i); *(uint32_t*)(tf + i) = *(const uint32_t*)(p.flags + i); }
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t i = base + j * BEAM_THREADS + tid;
                if (i >= v) continue;
                if (SCATTER) { p.count[i] = tc[i]; p.flags[i] = tf[i]; }
                else { tc[i] = p.count[i]; tf[i] = p.flags[i]; }
            }
        }
    }
    if (A.rows.dry) {
        const DryParam* p = A.rows.dry + slot;
        const uint32_t cap = p->cap;            // every slot of a call has the one window's capacity; the scratch rows are that long
        uint32_t* ring = p->ring;
        uint32_t* tr = A.tmp.ring + (size_t)q * cap;
        if (base < cap) {
            if ((cap & 3u) == 0) {
                const uint32_t i = base + tid * 4;
                if (i < cap) {
                    if (SCATTER) *(u32x4*)(ring + i) = *(const u32x4*)(tr + i);
                    else *(u32x4*)(tr + i) = *(const u32x4*)(ring + i);
                }
            } else {
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t i = base + j * BEAM_THREADS + tid;
                    if (i >= cap) continue;
                    if (SCATTER) ring[i] = tr[i]; else tr[i] = ring[i];
                }
            }
        }
        if (blockIdx.x == 0 && tid == 0) {
            uint32_t* tm = A.tmp.meta + (size_t)q * 2;
            if (SCATTER) { p->meta[0] = tm[0]; p->meta[1] = tm[1]; }
            else { tm[0] = p->meta[0]; tm[1] = p->meta[1]; }
        }
    }
    if (A.rows.gram && blockIdx.x == 0 && tid == 0) {
        if (SCATTER) A.rows.gram[q] = A.tmp.gram[q];
        else A.tmp.gram[q] = A.rows.gram[m];
    }
}

void beam_context_permute(hipStream_t s, const BeamCtxRows& rows, const BeamCtxScratch& scratch, uint32_t v, const uint32_t* map, uint32_t n) {
    if (n == 0 || (!rows.pen && !rows.dry && !rows.gram)) return;
    const BeamCtxArgs A{rows, scratch, map, v};
    const uint32_t longest = std::max(rows.pen ? v : 1u, rows.dry ? (uint32_t)WRK_MAX_TOKEN_WINDOW : 1u);
    const dim3 grid((longest + BEAM_CHUNK - 1) / BEAM_CHUNK, n);
    if (v % 4 == 0) {
        beam_context_kernel<true, false><<<grid, BEAM_THREADS, 0, s>>>(A);
        beam_context_kernel<true, true><<<grid, BEAM_THREADS, 0, s>>>(A);
    } else {
        beam_context_kernel<false, false><<<grid, BEAM_THREADS, 0, s>>>(A);
        beam_context_kernel<false, true><<<grid, BEAM_THREADS, 0, s>>>(A);
    }
}

int beam_step_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t b, const uint32_t* lp_tokens, const LogprobParam* lp,
                   LogprobPart* part, unsigned long long* keys, const BeamBufs& Q, uint32_t* tokens, uint32_t* counter, int num_cu) {
    if (b == 0) return 0;
    if (logprob_rows(s, logits, v, stride, b, lp_tokens, nullptr, lp, part, keys, num_cu) != 0) return -1;
    beam_select_kernel<<<1, BEAM_THREADS, 0, s>>>(Q, tokens, counter, b);
    return 0;
}

// slices of a layer's slot: layers * slices workgroups come to about two per CU, and no slice is smaller than one pass
void beam_copy(hipStream_t s, const BeamSlots& src, const BeamSlots& dst, uint32_t layers, size_t slot, const uint32_t* map, bool src_mapped,
               uint32_t n, int num_cu) {
    if (n == 0 || layers == 0 || slot == 0) return;
    BeamCopyArgs A{};
    A.src = src.base; A.dst = dst.base; A.src_nb = src.nb; A.src_b0 = src.b0; A.dst_nb = dst.nb; A.dst_b0 = dst.b0;
    A.map = map; A.src_mapped = src_mapped; A.layers = layers; A.slot = slot;
    A.vec = slot % 4 == 0 && (((uintptr_t)src.base | (uintptr_t)dst.base) & 15u) == 0;
    const uint32_t per_pass = A.vec ? BEAM_CHUNK : BEAM_THREADS;
    const uint32_t max_slices = (uint32_t)((slot + per_pass - 1) / per_pass);
    const uint32_t want = (2u * (uint32_t)num_cu + layers - 1) / layers;
    A.slices = want < 1 ? 1 : (want > max_slices ? max_slices : want);
    beam_copy_kernel<<<dim3(layers * A.slices, n), BEAM_THREADS, 0, s>>>(A);
}

void beam_permute(hipStream_t s, const BeamSlots& state, float* scratch, uint32_t layers, size_t slot, const uint32_t* map, uint32_t n, int num_cu) {
    const BeamSlots tmp{scratch, n, 0u};
    beam_copy(s, state, tmp, layers, slot, map, true, n, num_cu);
    beam_copy(s, tmp, state, layers, slot, map, false, n, num_cu);
}

}  // namespace wrk

int32_t wrk_beam_inv_norm(wrk_ctx* ctx, float length_penalty, uint32_t max_len, std::vector<float>& out) {
    WRK_ARG(ctx, finite_f32(length_penalty) && length_penalty >= 0.0f, "length_penalty %g: must be finite and >= 0", (double)length_penalty);
    out.assign((size_t)max_len + 1, 1.0f);
    for (uint32_t l = 1; l <= max_len; ++l) {
        out[l] = (float)(1.0 / pow((double)l, (double)length_penalty));
        WRK_ARG(ctx, std::isnormal(out[l]) && out[l] > 0.0f, "length_penalty %g: 1 / %u^penalty is not a normal f32", (double)length_penalty, l);
    }
    return WRK_OK;
}

int32_t wrk_beam_stops(wrk_ctx* ctx, const uint32_t* tokens, const uint32_t* off, uint32_t G, uint32_t V, std::vector<wrk::BeamStop>& rows) {
    WRK_ARG(ctx, !tokens || off, "stop_tokens without stop_offsets");
    rows.assign(G, wrk::BeamStop{});
    if (!off) return WRK_OK;
    WRK_ARG(ctx, off[0] == 0, "stop_offsets[0] = %u: must be 0", off[0]);
    for (uint32_t g = 0; g < G; ++g) {
        WRK_ARG(ctx, off[g + 1] >= off[g], "stop_offsets[%u] = %u decreases", g + 1, off[g + 1]);
        const uint32_t cnt = off[g + 1] - off[g];
        WRK_ARG(ctx, cnt <= WRK_MAX_BEAM_STOP_TOKENS, "group %u: %u stop tokens, at most %u", g, cnt, (uint32_t)WRK_MAX_BEAM_STOP_TOKENS);
        WRK_ARG(ctx, cnt == 0 || tokens, "stop_offsets name %u stop tokens, stop_tokens is NULL", cnt);
        for (uint32_t k = 0; k < cnt; ++k) {
            rows[g].ids[k] = tokens[off[g] + k];
            WRK_ARG(ctx, rows[g].ids[k] < V, "group %u: stop token %u >= vocab %u", g, rows[g].ids[k], V);
        }
        rows[g].count = cnt;
        std::sort(rows[g].ids, rows[g].ids + cnt);      // beam_is_stop searches them
    }
    return WRK_OK;
}

extern "C" int32_t wrk_beam_step(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t G, uint32_t W, float length_penalty,
                                 const uint32_t* stop_tokens, const uint32_t* stop_offsets, float* scores, float* keys, uint32_t* lengths,
                                 uint32_t* status, uint32_t* out_tokens, uint32_t* out_parents, uint32_t* out_copy_src) {
    if (!ctx || !logits) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, W >= 1 && W <= WRK_MAX_BEAMS, "num_beams %u: must be in [1, %u]", W, (uint32_t)WRK_MAX_BEAMS);
    WRK_ARG(ctx, G >= 1 && (uint64_t)G * W <= 256, "%u groups of %u beams: at most 256 slots", G, W);
    WRK_ARG(ctx, scores && keys && lengths && status && out_tokens && out_parents && out_copy_src, "every record and output array is required");
    const uint32_t B = G * W;
    int32_t rc = wrk_rows_check(ctx, logits, V, stride, B, "wrk_beam_step", wrk::SAMPLE_MAX_VOCAB);
    if (rc != WRK_OK) return rc;
    uint32_t max_len = 0;
    std::vector<wrk::BeamSlot> slots(B);
    for (uint32_t q = 0; q < B; ++q) {
        WRK_ARG(ctx, status[q] <= WRK_BEAM_DONE, "slot %u: status %u", q, status[q]);
        WRK_ARG(ctx, lengths[q] < 0x7fffffffu, "slot %u: length %u", q, lengths[q]);
        if (status[q] == WRK_BEAM_LIVE && lengths[q] + 1 > max_len) max_len = lengths[q] + 1;
        slots[q] = wrk::BeamSlot{scores[q], keys[q], lengths[q], status[q]};
    }
    std::vector<float> inv;
    std::vector<wrk::BeamStop> stops;
    rc = wrk_beam_inv_norm(ctx, length_penalty, max_len + 1, inv);
    if (rc == WRK_OK) rc = wrk_beam_stops(ctx, stop_tokens, stop_offsets, G, V, stops);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_par = dev.add(sizeof(wrk::BeamParam)), o_lpar = dev.add(sizeof(wrk::LogprobParam)), o_slots = dev.add((size_t)B * sizeof(wrk::BeamSlot));
    const size_t o_stops = dev.add((size_t)G * sizeof(wrk::BeamStop)), o_inv = dev.add(inv.size() * 4), o_ids = dev.add((size_t)B * W * 4);
    const size_t o_lp = dev.add((size_t)B * W * 4), o_chosen = dev.add((size_t)B * 4), o_part = dev.add(wrk::logprob_part_bytes(B));
    const size_t o_keys = dev.add(wrk::logprob_key_bytes(B)), o_hist = dev.add((size_t)3 * B * 4), o_maps = dev.add((size_t)4 * B * 4);
    const size_t o_words = dev.add(8), o_tok = dev.add((size_t)2 * B * 4);
    WRK_HIP(ctx, dev.alloc());
    const wrk::BeamParam par{W, G, 1u, (uint32_t)inv.size()};
    const wrk::LogprobParam lpar{dev.at<float>(o_chosen), dev.at<uint32_t>(o_ids), dev.at<float>(o_lp), W, B};
    uint32_t* hist = dev.at<uint32_t>(o_hist);
    uint32_t* maps = dev.at<uint32_t>(o_maps);
    uint32_t* words = dev.at<uint32_t>(o_words);        // the LIVE count, the step counter
    uint32_t* tok = dev.at<uint32_t>(o_tok);            // [B] zeros: the chosen tokens of the front; [B] the tokens the slots feed
    const wrk::BeamBufs Q{dev.at<wrk::BeamParam>(o_par), dev.at<wrk::BeamSlot>(o_slots), dev.at<wrk::BeamStop>(o_stops), dev.at<float>(o_inv),
                          lpar.top_ids, lpar.top_logprobs, hist, hist + B, (float*)(hist + 2 * B), maps, maps + B, maps + 2 * B, words, maps + 3 * B};
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), &par, sizeof par, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_lpar), &lpar, sizeof lpar, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_slots), slots.data(), (size_t)B * sizeof(wrk::BeamSlot), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_stops), stops.data(), (size_t)G * sizeof(wrk::BeamStop), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_inv), inv.data(), inv.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemsetAsync(words, 0, 8, ctx->stream));
    WRK_HIP(ctx, hipMemsetAsync(tok, 0, (size_t)2 * B * 4, ctx->stream));
    if (wrk::beam_step_rows(ctx->stream, (const float*)logits->ptr, V, stride, B, tok, dev.at<wrk::LogprobParam>(o_lpar), dev.at<wrk::LogprobPart>(o_part),
                            dev.at<unsigned long long>(o_keys), Q, tok + B, words + 1, ctx->num_cu) != 0)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "wrk_beam_step: vocabulary of %u tokens", V);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(slots.data(), Q.slots, (size_t)B * sizeof(wrk::BeamSlot), hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(out_tokens, Q.step_tokens, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(out_parents, Q.step_parents, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(out_copy_src, Q.copy_src, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t q = 0; q < B; ++q) { scores[q] = slots[q].score; keys[q] = slots[q].key; lengths[q] = slots[q].length; status[q] = slots[q].status; }
    return WRK_OK;
}

extern "C" int32_t wrk_v7_state_permute(wrk_ctx* ctx, wrk_v7_state* st, const uint32_t* parents, uint32_t n) {
    if (!ctx || !st) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_v7_state_permute is blocking: not inside a capture");
    WRK_ARG(ctx, st->ctx == ctx, "the state belongs to another context");
    WRK_ARG(ctx, n <= st->num_batch, "%u slots, the state has %u", n, st->num_batch);
    if (n == 0) return WRK_OK;
    WRK_ARG(ctx, parents, "parents is required");
    std::vector<uint32_t> map(n);
    bool any = false;
    for (uint32_t q = 0; q < n; ++q) {
        WRK_ARG(ctx, parents[q] < n, "parents[%u] = %u: must be below %u", q, parents[q], n);
        map[q] = parents[q] == q ? WRK_BEAM_NO_COPY : parents[q];
        any = any || parents[q] != q;
    }
    if (!any) return WRK_OK;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t slot = (size_t)(st->head_size + 2) * st->num_emb;
    wrk_dev_arena dev;
    const size_t o_map = dev.add((size_t)n * 4), o_tmp = dev.add((size_t)st->num_layer * n * slot * 4);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_map), map.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::beam_permute(ctx->stream, wrk::BeamSlots{st->data, st->num_batch, 0u}, dev.at<float>(o_tmp), st->num_layer, slot, dev.at<uint32_t>(o_map), n,
                      ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// parents of wrk_occurrence_permute / wrk_token_window_permute validated into a copy list (WRK_E_ARG as wrk_v7_state_permute); *any:
// whether a slot moves at all
static int32_t beam_parents_map(wrk_ctx* ctx, const uint32_t* parents, uint32_t n, uint32_t num_batch, const char* who, std::vector<uint32_t>& map, bool* any) {
    WRK_ARG(ctx, !ctx->capturing_here(), "%s is blocking: not inside a capture", who);
    WRK_ARG(ctx, n <= num_batch, "%u slots, %s has %u", n, who, num_batch);
    *any = false;
    if (n == 0) return WRK_OK;
    WRK_ARG(ctx, parents, "parents is required");
    map.resize(n);
    for (uint32_t q = 0; q < n; ++q) {
        WRK_ARG(ctx, parents[q] < n, "parents[%u] = %u: must be below %u", q, parents[q], n);
        map[q] = parents[q] == q ? WRK_BEAM_NO_COPY : parents[q];
        *any = *any || parents[q] != q;
    }
    return WRK_OK;
}

extern "C" int32_t wrk_occurrence_permute(wrk_ctx* ctx, wrk_occurrence* occ, const uint32_t* parents, uint32_t n) {
    if (!ctx || !occ) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, occ->ctx == ctx, "the occurrence table belongs to another context");
    std::vector<uint32_t> map;
    bool any = false;
    const int32_t rc = beam_parents_map(ctx, parents, n, occ->num_batch, "the occurrence table", map, &any);
    if (rc != WRK_OK || !any) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t V = occ->num_vocab;
    std::vector<wrk::PenaltyParam> rows(n);
    for (uint32_t q = 0; q < n; ++q) rows[q] = occ->row(q, 0.0f, 0.0f, 1.0f);
    wrk_dev_arena dev;
    const size_t o_map = dev.add((size_t)n * 4), o_rows = dev.add((size_t)n * sizeof(wrk::PenaltyParam)), o_cnt = dev.add((size_t)n * V * 4),
                 o_flg = dev.add((size_t)n * V);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_map), map.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_rows), rows.data(), (size_t)n * sizeof(wrk::PenaltyParam), hipMemcpyHostToDevice, ctx->stream));
    wrk::beam_context_permute(ctx->stream, wrk::BeamCtxRows{dev.at<wrk::PenaltyParam>(o_rows), nullptr, nullptr},
                              wrk::BeamCtxScratch{dev.at<float>(o_cnt), dev.at<uint8_t>(o_flg), nullptr, nullptr, nullptr}, occ->num_vocab,
                              dev.at<uint32_t>(o_map), n);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

extern "C" int32_t wrk_token_window_permute(wrk_ctx* ctx, wrk_token_window* win, const uint32_t* parents, uint32_t n) {
    if (!ctx || !win) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, win->ctx == ctx, "the token window belongs to another context");
    std::vector<uint32_t> map;
    bool any = false;
    const int32_t rc = beam_parents_map(ctx, parents, n, win->num_batch, "the token window", map, &any);
    if (rc != WRK_OK || !any) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<wrk::DryParam> rows(n);
    for (uint32_t q = 0; q < n; ++q) {
        rows[q].ring = win->ring + (size_t)q * win->capacity;
        rows[q].meta = win->meta + (size_t)q * 2;
        rows[q].cap = win->capacity;
    }
    wrk_dev_arena dev;
    const size_t o_map = dev.add((size_t)n * 4), o_rows = dev.add((size_t)n * sizeof(wrk::DryParam)), o_ring = dev.add((size_t)n * win->capacity * 4),
                 o_meta = dev.add((size_t)n * 8);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_map), map.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_rows), rows.data(), (size_t)n * sizeof(wrk::DryParam), hipMemcpyHostToDevice, ctx->stream));
    wrk::beam_context_permute(ctx->stream, wrk::BeamCtxRows{nullptr, dev.at<wrk::DryParam>(o_rows), nullptr},
                              wrk::BeamCtxScratch{nullptr, nullptr, dev.at<uint32_t>(o_ring), dev.at<uint32_t>(o_meta), nullptr}, win->num_vocab,
                              dev.at<uint32_t>(o_map), n);
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}
