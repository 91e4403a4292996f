// Host-side driver shared by the RWKV-7 and RWKV-6 runners (wrk_runner.h).  No kernels here.
#include "wrk_runner.h"

#include <algorithm>

#define LOCK(ctx) std::lock_guard<std::recursive_mutex> _lk((ctx)->mu)

// ------------------------------------------------------------------ matmul launches
wrk::MatJob wrk::mat_job(const wrk_matrix* m, DTensor in, DTensor out, uint32_t act) {
    wrk::MatJob j{m->data, m->aux, m->kind, m->flags, m->k, m->m, (uint32_t)m->row_bytes, in, out, act, 0};
    j.scale = m->out_scale;
    return j;
}

int32_t wrk_mm(wrk_ctx* ctx, const wrk_matrix* m, DTensor in, DTensor out, uint32_t act) {
    wrk::MatJob j = wrk::mat_job(m, in, out, act);
    return wrk_mm_group(ctx, &j, 1);
}

int32_t wrk_mm_group(wrk_ctx* ctx, wrk::MatJob* jobs, int n) {
    // scratch of the third-generation prefill tile: a launch reads it from its first job, and every job may lead a launch of its own in the
    // per-matrix leg
    const wrk::T3Scratch t3{ctx->gemm_scratch, ctx->gemm_scratch_cap};
    for (int i = 1; i < n; ++i) { jobs[i].xsum = t3.p; jobs[i].xsum_cap = t3.cap; }
    int bad = 0;
    const int rc = wrk::matmul_jobs(ctx->op_stream(), jobs, n, jobs[0].in.shape[1] * jobs[0].in.shape[2], ctx->num_cu, nullptr, &t3, wrk::FewTokens::matvec_each, &bad);
    if (rc != 0) return wrk_fail(ctx, WRK_E_ARG, "matmul launch rejected (K=%u M=%u rc=%d)", jobs[bad].k, jobs[bad].m, rc);
    return WRK_OK;
}

int32_t wrk_buf_write_raw(wrk_ctx* ctx, void* dst, const void* src, size_t bytes) {
    wrk_buf tmp{ctx, dst, bytes, {1}};
    return wrk_buf_write(ctx, &tmp, 0, src, bytes);
}

// the uploads of a prepare function: up(dst, src, n) writes n elements of T from the host to the device, nothing after the first error
struct wrk_upload {
    wrk_ctx* ctx;
    int32_t rc = WRK_OK;
    template <class T> wrk_upload& operator()(T* dst, const T* src, size_t n) {
        if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, dst, src, n * sizeof(T));
        return *this;
    }
};

// ------------------------------------------------------------------ job validation
int32_t wrk_job_check(wrk_ctx* ctx, const wrk_v7_state* st, const uint32_t* cursors, uint32_t T, const uint32_t* tokens, uint32_t V,
                      const uint32_t* headers, uint32_t NH, wrk_job_shape* shape) {
    wrk_job_shape sh{0, true, true, NH == T};
    std::vector<uint8_t> seen(256, 0);
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t c = cursors[t], b = c & 0xff, tok = (c >> 8) & 0xffff, len = c >> 24;
        WRK_ARG(ctx, b < st->num_batch, "cursor %u: batch %u >= %u", t, b, st->num_batch);
        WRK_ARG(ctx, len >= 1 && tok <= t && t < tok + len && tok + len <= T, "cursor %u: bad range (token %u len %u)", t, tok, len);
        if (tok == t) {
            ++sh.nseq;
            WRK_ARG(ctx, !seen[b], "cursor %u: batch %u appears in two chunks of one dispatch", t, b);   // two writers of one state slice
            seen[b] = 1;
        }
        if (len != 1) sh.one_token_each = false;
        if (tokens) WRK_ARG(ctx, tokens[t] < V, "token %u: id %u >= vocab %u", t, tokens[t], V);
        // batches of consecutive tokens are consecutive: the few-sequence decode kernels address per-sequence state rows by a stride
        if (b != (cursors[0] & 0xff) + t) sh.contiguous = false;
    }
    for (uint32_t h = 0; h < NH; ++h) {
        WRK_ARG(ctx, headers[h] < T, "header %u: row %u >= %u tokens", h, headers[h], T);
        if (headers[h] != h) sh.identity = false;
    }
    *shape = sh;
    return WRK_OK;
}

int32_t wrk_score_check(wrk_ctx* ctx, const wrk_job_args& a, uint32_t V, const char* who) {
    if (!a.score) return WRK_OK;
    WRK_ARG(ctx, !ctx->capturing_here(), "%s is blocking: not inside a capture", who);
    WRK_ARG(ctx, a.NH == 0 || (a.logprob && a.rank), "logprob and rank are required");
    return wrk_score_check_targets(ctx, a.targets, a.NH, V);
}

// ------------------------------------------------------------------ frame state
void wrk_frame_common::drop_graphs() {
    for (auto& kv : graphs) wrk_program_destroy(kv.second);
    graphs.clear();
}

int32_t wrk_frame_common::ensure_poll(uint32_t lanes) {
    if (live_host_cap < 2 * lanes) {
        if (live_host) hipHostFree(live_host);
        live_host = nullptr; live_host_cap = 0;
        WRK_HIP(ctx, hipHostMalloc((void**)&live_host, (size_t)2 * lanes * 4, hipHostMallocDefault));
        live_host_cap = 2 * lanes;
    }
    while (poll_events.size() < (size_t)2 * lanes) {
        hipEvent_t e = nullptr;
        WRK_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        poll_events.push_back(e);
    }
    return WRK_OK;
}

void wrk_frame_common::release_common() {
    drop_graphs();
    if (scratch) hipFree(scratch);
    scratch = nullptr;
    each_group([](auto& g) { g.release(); });
    if (live_host) hipHostFree(live_host);
    live_host = nullptr; live_host_cap = 0;
    for (hipEvent_t e : poll_events) hipEventDestroy(e);
    poll_events.clear();
}

int32_t wrk_cached_program(wrk_ctx* ctx, std::map<wrk_frame_common::GraphKey, wrk_program*>& graphs, const wrk_frame_common::GraphKey& key,
                           const std::function<int32_t()>& enqueue, wrk_program** prog) {
    auto it = graphs.find(key);
    if (it != graphs.end()) { *prog = it->second; return WRK_OK; }
    int32_t rc = wrk_capture_begin(ctx);
    if (rc != WRK_OK) return rc;
    rc = enqueue();
    wrk_program* p = nullptr;
    const int32_t rc2 = wrk_capture_end(ctx, &p);
    if (rc != WRK_OK) { if (p) wrk_program_destroy(p); return rc; }
    if (rc2 != WRK_OK) return rc2;
    graphs[key] = p;
    *prog = p;
    return WRK_OK;
}

// ------------------------------------------------------------------ job upload / read-back
int32_t wrk_job_upload(wrk_frame_common& f, wrk::FrameIo& io, void* input, const wrk_buf* emb, uint32_t D, const wrk_job_args& a, bool gather) {
    wrk_ctx* ctx = f.ctx;
    int32_t rc = WRK_OK;
    if (a.score && a.NH) {
        rc = f.grow(f.score, {a.NH});          // captured score jobs hold the old slots: they go when the slots move
        if (rc != WRK_OK) return rc;
        rc = wrk_buf_write_raw(ctx, f.score.targets, a.targets, (size_t)a.NH * 4);
    }
    if (rc == WRK_OK) rc = wrk_buf_write_raw(ctx, io.cursors, a.cursors, (size_t)a.T * 4);
    if (rc == WRK_OK && a.NH) rc = wrk_buf_write_raw(ctx, io.headers, a.headers, (size_t)a.NH * 4);
    if (rc != WRK_OK) return rc;
    if (!a.tokens) return wrk_buf_write_raw(ctx, input, a.emb_rows, (size_t)a.T * D * 2);
    rc = wrk_buf_write_raw(ctx, io.tokens, a.tokens, (size_t)a.T * 4);
    if (rc == WRK_OK && gather) wrk::gather_rows_f16(ctx->op_stream(), emb->ptr, io.tokens, input, D, a.T);
    return rc;
}

int32_t wrk_job_read_back(wrk_frame_common& f, const wrk::FrameIo& io, uint32_t V, const wrk_job_args& a) {
    wrk_ctx* ctx = f.ctx;
    WRK_LAUNCH_CHECK(ctx);
    if (ctx->capturing_here()) return WRK_OK;   // recorded into the caller's program: results exist after it has been launched
    if (a.NH && a.logits) WRK_HIP(ctx, hipMemcpyAsync(a.logits, io.head_o, (size_t)a.NH * V * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (a.NH && a.argmax) WRK_HIP(ctx, hipMemcpyAsync(a.argmax, io.argmax, (size_t)a.NH * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (a.NH && a.score) {
        WRK_HIP(ctx, hipMemcpyAsync(a.logprob, f.score.logprob, (size_t)a.NH * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(a.rank, f.score.rank, (size_t)a.NH * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// ------------------------------------------------------------------ decode loops: validation and upload
struct wrk_pick_params {    // validated rows; empty: the arg-max / without penalties / without filters
    std::vector<wrk::SampleParam> par; std::vector<wrk::PenaltyParam> pen; std::vector<wrk::SampleFilter> filt;
    std::vector<wrk::SampleAlt> alt;        // Mirostat / typical rows
    std::vector<wrk::SampleCut> cut;        // the cut sampler's rows, next to filt (which a cut pick always has)
    const wrk_grammar* grammar = nullptr;   // a constrained pick: the automaton and the state every row starts in
    std::vector<uint32_t> gram_state;
    const wrk_logit_bias* bias = nullptr;   // a biased pick: the object and every row's set word
    std::vector<uint32_t> bias_set;
    bool has_dry = false;                   // a DRY pick: the rows' window slots, values and tables, and the call's breakers
    std::vector<wrk::DryParam> dry;
    wrk::DryBreakers brk{};
    std::vector<float> guide;               // a guided call: the scales of its R sequences (wrk_guide_pack); the frame then runs 2R
};

// The one validation of the pick arrays (wrk_pick_args).  Sets kind.pick / kind.penalized and packs `n` rows; penalty row r names slot r
// of the table for r < slots (the table must have `slots`), slot 0 beyond: the queue keeps only the values of its request rows
static int32_t wrk_pick_pack(wrk_ctx* ctx, const wrk_pick_args& a, uint32_t n, uint32_t slots, uint32_t V, wrk_pick_params& out, wrk_step_kind& kind) {
    const int given = (a.temperature != nullptr) + (a.top_p != nullptr) + (a.seed != nullptr);
    WRK_ARG(ctx, given == 3 || (given == 0 && a.need == wrk_pick_args::ANY), "temperature, top_p and seed: all three arrays%s",
            a.need == wrk_pick_args::ANY ? ", or none for the arg-max" : "");
    WRK_ARG(ctx, a.occ || a.need != wrk_pick_args::TABLE, "occurrence table required");
    WRK_ARG(ctx, a.occ || (!a.presence && !a.frequency && !a.decay), "penalty arrays without an occurrence table");
    WRK_ARG(ctx, !a.occ || given == 3, "penalties need the sampler arrays");
    WRK_ARG(ctx, (!a.top_k && !a.min_p) || given == 3, "top_k / min_p need the sampler arrays");
    const bool cut = a.cut.any();
    const bool filt = a.top_k || a.min_p || cut, miro = a.mirostat_tau || a.mirostat_eta || a.mirostat_mu, typ = a.typical_p != nullptr;
    WRK_ARG(ctx, !cut || given == 3, "top_n_sigma / epsilon_cutoff / eta_cutoff / xtc_* need the sampler arrays");
    WRK_ARG(ctx, !miro || a.mirostat_tau, "mirostat_eta / mirostat_mu without mirostat_tau");
    WRK_ARG(ctx, (int)filt + (int)miro + (int)typ <= 1, "one family per call: top_k / min_p and the cuts, mirostat_* or typical_p");
    WRK_ARG(ctx, (!miro && !typ) || given == 3, "mirostat_* / typical_p need the sampler arrays");
    kind.pick = given == 0 ? wrk_step_kind::GREEDY : cut ? wrk_step_kind::CUT : filt ? wrk_step_kind::FILTERED : miro ? wrk_step_kind::MIROSTAT
                           : typ ? wrk_step_kind::TYPICAL : wrk_step_kind::SAMPLED;
    kind.penalized = a.occ != nullptr;
    WRK_ARG(ctx, a.grammar || !a.grammar_state, "grammar_state without grammar");
    kind.constrained = a.grammar != nullptr;
    if (kind.constrained) {
        const int32_t grc = wrk_grammar_pack(ctx, a.grammar, a.grammar_state, n, V, out.gram_state);
        if (grc != WRK_OK) return grc;
        out.grammar = a.grammar;
    }
    WRK_ARG(ctx, a.bias || !a.bias_set, "bias_set without bias");
    kind.biased = a.bias != nullptr;
    if (kind.biased) {
        const int32_t brc = wrk_bias_pack(ctx, a.bias, a.bias_set, n, V, out.bias_set);
        if (brc != WRK_OK) return brc;
        out.bias = a.bias;
    }
    WRK_ARG(ctx, a.dry.window || !a.dry.any_array(), "dry_* / no_repeat_ngram arrays without a token window");
    kind.dry = a.dry.window != nullptr;
    if (kind.dry) {
        const int32_t drc = wrk_dry_pack(ctx, a.dry, 0, n, slots, V, out.dry, out.brk);
        if (drc != WRK_OK) return drc;
        WRK_ARG(ctx, a.dry.window->num_batch >= slots, "token window of %u slots, %u state slots", a.dry.window->num_batch, slots);
        out.has_dry = true;
    }
    if (!kind.sampled()) return WRK_OK;
    WRK_ARG(ctx, n >= 1, "a sampled pick of no rows");
    int32_t rc = wrk_sample_pack(ctx, a.temperature, a.top_p, a.seed, n, out.par);
    if (rc == WRK_OK && kind.filtered()) rc = wrk_filter_pack(ctx, a.top_k, a.min_p, n, out.filt);
    if (rc == WRK_OK && kind.cut()) rc = wrk_cut_pack(ctx, a.cut, n, out.cut);
    if (rc == WRK_OK && kind.cut() && V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "sampler: vocabulary of %u tokens", V);
    if (rc == WRK_OK && miro) rc = wrk_mirostat_pack(ctx, a.mirostat_tau, a.mirostat_eta, a.mirostat_mu, n, out.alt);
    if (rc == WRK_OK && typ) rc = wrk_typical_pack(ctx, a.typical_p, n, out.alt);
    if (rc == WRK_OK && kind.alt() && V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "sampler: vocabulary of %u tokens", V);
    if (rc != WRK_OK || !kind.penalized) return rc;
    WRK_ARG(ctx, a.decay, "decay array required");
    WRK_ARG(ctx, a.occ->num_batch >= slots, "occurrence table of %u slots, %u state slots", a.occ->num_batch, slots);
    // the rows that name a slot of their own in one call, so that a bad value is reported with its row; request rows beyond the slots
    // (a queue of more requests than slots) one at a time on slot 0
    const uint32_t own = n < slots ? n : slots;
    rc = wrk_penalty_pack(ctx, a.occ, 0, own, V, a.presence, a.frequency, a.decay, out.pen);
    std::vector<wrk::PenaltyParam> one;
    for (uint32_t r = own; r < n && rc == WRK_OK; ++r) {
        rc = wrk_penalty_pack(ctx, a.occ, 0, 1, V, a.presence ? a.presence + r : nullptr, a.frequency ? a.frequency + r : nullptr, a.decay + r, one);
        if (rc == WRK_OK) out.pen.push_back(one[0]);
    }
    return rc;
}

// a stop-set CSR over n owners ("sequence", "request") validated into rows [n] (ids, count); both arrays NULL: all empty
static int32_t wrk_stop_sets(wrk_ctx* ctx, const uint32_t* tokens, const uint32_t* off, uint32_t n, uint32_t V, const char* owner,
                               std::vector<wrk::StopParam>& rows) {
    WRK_ARG(ctx, !tokens || off, "stop_tokens without stop_offsets");
    rows.assign(n, wrk::StopParam{});
    if (!off) return WRK_OK;
    WRK_ARG(ctx, off[0] == 0, "stop_offsets[0] = %u: must be 0", off[0]);
    for (uint32_t i = 0; i < n; ++i) {
        WRK_ARG(ctx, off[i + 1] >= off[i], "stop_offsets[%u] = %u decreases", i + 1, off[i + 1]);
        const uint32_t cnt = off[i + 1] - off[i];
        WRK_ARG(ctx, cnt <= WRK_MAX_STOP_TOKENS, "%s %u: %u stop tokens, at most %u", owner, i, cnt, (uint32_t)WRK_MAX_STOP_TOKENS);
        WRK_ARG(ctx, cnt == 0 || tokens, "stop_offsets name %u stop tokens, stop_tokens is NULL", cnt);
        for (uint32_t k = 0; k < cnt; ++k) {
            rows[i].ids[k] = tokens[off[i] + k];
            WRK_ARG(ctx, rows[i].ids[k] < V, "%s %u: stop token %u >= vocab %u", owner, i, rows[i].ids[k], V);
        }
        rows[i].count = cnt;
    }
    return WRK_OK;
}

// The stop-sequence arrays of a call over n owners ("sequence", "request", "row"), validated (WRK_E_ARG before any launch)
// into device rows [n], every sequence reversed as wrk::StopSeqRow says, and tails [n][WRK_STOP_TAIL_LEN] (tail_in NULL: empty).  on:
// the three arrays are given -- the call runs stop-sequence programs, whatever they hold.  has_out: the call passed out_stop_match or
// stop_tail, which need the arrays
struct wrk_stopseq_pack {
    bool on = false;
    std::vector<wrk::StopSeqRow> rows;
    std::vector<uint32_t> tails;
};
static int32_t wrk_stop_seqs(wrk_ctx* ctx, const uint32_t* tokens, const uint32_t* off, const uint32_t* owners, bool has_out, const uint32_t* tail_in,
                             uint32_t n, uint32_t V, const char* owner, wrk_stopseq_pack& pk) {
    const int given = (tokens != nullptr) + (off != nullptr) + (owners != nullptr);
    WRK_ARG(ctx, given == 0 || given == 3, "stop_seq_tokens, stop_seq_offsets and stop_seq_owners: all three arrays, or none");
    pk.on = given == 3;
    WRK_ARG(ctx, pk.on || !has_out, "out_stop_match / stop_tail without the stop-sequence arrays");
    if (!pk.on) return WRK_OK;
    pk.rows.assign(n, wrk::StopSeqRow{});
    pk.tails.assign((size_t)n * WRK_STOP_TAIL_LEN, WRK_STOP_TAIL_EMPTY);
    WRK_ARG(ctx, owners[0] == 0, "stop_seq_owners[0] = %u: must be 0", owners[0]);
    WRK_ARG(ctx, off[0] == 0, "stop_seq_offsets[0] = %u: must be 0", off[0]);
    for (uint32_t i = 0; i < n; ++i) {
        WRK_ARG(ctx, owners[i + 1] >= owners[i], "stop_seq_owners[%u] = %u decreases", i + 1, owners[i + 1]);
        const uint32_t cnt = owners[i + 1] - owners[i];
        WRK_ARG(ctx, cnt <= WRK_MAX_STOP_SEQUENCES, "%s %u: %u stop sequences, at most %u", owner, i, cnt, (uint32_t)WRK_MAX_STOP_SEQUENCES);
        wrk::StopSeqRow& row = pk.rows[i];
        row.count = cnt;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t s = owners[i] + k;
            WRK_ARG(ctx, off[s + 1] >= off[s], "stop_seq_offsets[%u] = %u decreases", s + 1, off[s + 1]);
            const uint32_t l = off[s + 1] - off[s];
            WRK_ARG(ctx, l >= 1 && l <= WRK_MAX_STOP_SEQUENCE_LEN, "%s %u: stop sequence %u has %u ids, 1 to %u", owner, i, k, l,
                    (uint32_t)WRK_MAX_STOP_SEQUENCE_LEN);
            row.len[k] = l;
            for (uint32_t j = 0; j < l; ++j) {
                const uint32_t id = tokens[off[s] + j];
                WRK_ARG(ctx, id < V, "%s %u: stop sequence %u holds id %u >= vocab %u", owner, i, k, id, V);
                row.tok[k][l - 1 - j] = id;
            }
        }
    }
    for (size_t i = 0; tail_in && i < pk.tails.size(); ++i) {
        const uint32_t t = tail_in[i];
        WRK_ARG(ctx, t == WRK_STOP_TAIL_EMPTY || t < V, "stop_tail[%zu] = %u: neither EMPTY nor < vocab %u", i, t, V);
        WRK_ARG(ctx, t != WRK_STOP_TAIL_EMPTY || i % WRK_STOP_TAIL_LEN == 0 || tail_in[i - 1] == WRK_STOP_TAIL_EMPTY,
                "stop_tail[%zu]: EMPTY after an id (a tail is right aligned)", i);
        pk.tails[i] = t;
    }
    return WRK_OK;
}

extern "C" int32_t wrk_stop_sequences_advance(wrk_ctx* ctx, uint32_t V, uint32_t n, const uint32_t* seq_tokens, const uint32_t* seq_offsets,
                                              const uint32_t* seq_owners, const uint32_t* stop_tokens, const uint32_t* stop_offsets, uint32_t* tails,
                                              const uint32_t* tokens, uint32_t* out_match) {
    if (!ctx) return WRK_E_ARG;
    LOCK(ctx);
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_stop_sequences_advance is blocking: not inside a capture");
    WRK_ARG(ctx, seq_tokens && seq_offsets && seq_owners, "stop_seq_tokens, stop_seq_offsets and stop_seq_owners are required");
    WRK_ARG(ctx, n == 0 || (tails && tokens && out_match), "tails, tokens and out_match are required");
    wrk_stopseq_pack pk;
    std::vector<wrk::StopParam> ids;
    int32_t rc = wrk_stop_seqs(ctx, seq_tokens, seq_offsets, seq_owners, true, tails, n, V, "row", pk);
    if (rc == WRK_OK) rc = wrk_stop_sets(ctx, stop_tokens, stop_offsets, n, V, "row", ids);
    if (rc != WRK_OK || n == 0) return rc;
    for (uint32_t r = 0; r < n; ++r) WRK_ARG(ctx, tokens[r] < V, "token %u: id %u >= vocab %u", r, tokens[r], V);
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_rows = dev.add((size_t)n * sizeof(wrk::StopSeqRow)), o_ids = dev.add((size_t)n * sizeof(wrk::StopParam)),
                 o_tail = dev.add((size_t)n * WRK_STOP_TAIL_LEN * 4), o_tok = dev.add((size_t)n * 4), o_match = dev.add((size_t)n * 4);
    WRK_HIP(ctx, dev.alloc());
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_rows), pk.rows.data(), (size_t)n * sizeof(wrk::StopSeqRow), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_ids), ids.data(), (size_t)n * sizeof(wrk::StopParam), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tail), pk.tails.data(), pk.tails.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_tok), tokens, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    wrk::stop_seq_rows(ctx->stream, n, dev.at<wrk::StopSeqRow>(o_rows), dev.at<wrk::StopParam>(o_ids), dev.at<uint32_t>(o_tail), dev.at<uint32_t>(o_tok),
                       dev.at<uint32_t>(o_match));
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(tails, dev.at<char>(o_tail), pk.tails.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(out_match, dev.at<char>(o_match), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// the log-prob fields of an options struct validated (WRK_E_ARG / WRK_E_UNSUPPORTED before any launch); sets kind.logprobs
static int32_t wrk_logprob_check(wrk_ctx* ctx, const wrk_logprob_call& lp, uint32_t V, wrk_step_kind& kind) {
    kind.logprobs = lp.on();
    WRK_ARG(ctx, lp.num_top <= WRK_MAX_TOP_LOGPROBS, "num_top %u: at most %u", lp.num_top, (uint32_t)WRK_MAX_TOP_LOGPROBS);
    if (!lp.on()) {
        WRK_ARG(ctx, !lp.top_ids && !lp.top_logprobs, "top_ids / top_logprobs without logprob");
        return WRK_OK;
    }
    WRK_ARG(ctx, lp.num_top == 0 || (lp.top_ids && lp.top_logprobs), "top_ids and top_logprobs are required with num_top > 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "log-probs: vocabulary of %u tokens", V);
    return WRK_OK;
}

// after wrk_decode_prepare and before the step program is looked up (growing the buffers drops the programs): the frame's log-prob
// buffers for `steps` steps of B sequences and the parameter block of this call
static int32_t wrk_logprob_prepare(wrk_frame_common& f, uint32_t B, uint32_t steps, uint32_t num_top) {
    const int32_t rc = f.grow(f.logprob, {(size_t)steps * B, B});
    if (rc != WRK_OK) return rc;
    const wrk::LogprobParam par{f.logprob.logprob, f.logprob.top_ids, f.logprob.top_logprobs, num_top, (uint32_t)((size_t)steps * B)};
    wrk_upload up{f.ctx};
    if (up(f.logprob.par, &par, 1).rc != WRK_OK) return up.rc;
    WRK_HIP(f.ctx, hipStreamSynchronize(f.ctx->stream));
    return WRK_OK;
}

bool wrk_no_graph() {
    const char* e = getenv("WRK_NO_GRAPH");
    return e && e[0] == '1';
}

static int32_t wrk_generate_check(wrk_ctx* ctx, const wrk_v7_state* st, const wrk_frame_common::Facts& m, const uint32_t* first_tokens, uint32_t B) {
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    WRK_ARG(ctx, m.has_emb, "generate_greedy needs the device embedding table");
    WRK_ARG(ctx, B >= 1 && B <= st->num_batch, "num_batch %u exceeds the state's %u", B, st->num_batch);
    WRK_ARG(ctx, st->num_emb == m.num_emb && st->num_layer == m.num_layer, "state does not belong to this model");
    for (uint32_t b = 0; b < B; ++b) WRK_ARG(ctx, first_tokens[b] < m.num_vocab, "first token %u out of vocab", first_tokens[b]);
    return WRK_OK;
}

// after the runner's ensure_frame: history / parameter buffers, then cursors, header rows, first_tokens [b0, b0 + B) and rows
// [b0, b0 + B) of `rows` for sequences [b0, b0 + B), and a zero step counter.  A guided call (rows.guide): B = 2R sequences of the
// frame, the pick rows and the scales of the R conditional ones
static int32_t wrk_decode_prepare(wrk_frame_common& f, const uint32_t* first_tokens, uint32_t b0, uint32_t B, uint32_t steps, const wrk_pick_params& rows) {
    wrk_ctx* ctx = f.ctx;
    wrk::FrameIo& io = f.io();
    const wrk::SampleParam* par = rows.par.empty() ? nullptr : rows.par.data() + b0;
    const wrk::PenaltyParam* pen = rows.pen.empty() ? nullptr : rows.pen.data() + b0;
    const wrk::SampleFilter* filt = rows.filt.empty() ? nullptr : rows.filt.data() + b0;
    const wrk::SampleAlt* alt = rows.alt.empty() ? nullptr : rows.alt.data() + b0;
    const wrk::SampleCut* cut = rows.cut.empty() ? nullptr : rows.cut.data() + b0;
    const size_t V = f.facts().num_vocab;
    const bool guided = !rows.guide.empty();
    const uint32_t R = guided ? B / 2 : B;      // rows of the pick
    int32_t rc = f.grow(f.history, {(size_t)steps * B});
    if (rc == WRK_OK && par) rc = f.grow(f.sample, {R});
    if (rc == WRK_OK && filt) rc = f.grow(f.filter, {R});
    if (rc == WRK_OK && alt) rc = f.grow(f.alt, {R});
    if (rc == WRK_OK && cut) rc = f.grow(f.cut_par, {R});
    if (rc == WRK_OK && pen) rc = f.grow(f.penalty, {R, V});
    if (rc == WRK_OK && rows.grammar) rc = f.grow(f.grammar, {R, V});
    if (rc == WRK_OK && rows.bias) rc = f.grow(f.bias, {R, V});
    if (rc == WRK_OK && guided) rc = f.grow(f.guide, {R, V});
    if (rc == WRK_OK && rows.has_dry) rc = f.grow(f.dry, {R, V});
    if (rc != WRK_OK) return rc;
    std::vector<uint32_t> cur(B), hdr(B);
    for (uint32_t b = 0; b < B; ++b) { cur[b] = (b0 + b) | (b << 8) | (1u << 24); hdr[b] = b; }
    wrk_upload up{ctx};
    up(io.cursors, cur.data(), B)(io.headers, hdr.data(), B)(io.tokens, first_tokens + b0, B);
    if (par) up(f.sample.par, par, R);
    if (filt) up(f.filter.par, filt, R);
    if (alt) up(f.alt.par, alt, R);
    if (cut) up(f.cut_par.par, cut, R);
    if (pen) up(f.penalty.par, pen, R);
    if (rows.grammar) {
        const wrk::GrammarParam gp = rows.grammar->param(f.grammar.state);
        up(f.grammar.par, &gp, 1)(f.grammar.state, rows.gram_state.data() + b0, R);
    }
    if (rows.bias) {
        const wrk::BiasParam bp = rows.bias->param(f.bias.set);
        up(f.bias.par, &bp, 1)(f.bias.set, rows.bias_set.data() + b0, R);
    }
    if (guided) up(f.guide.par, rows.guide.data() + b0, R);
    if (rows.has_dry) {
        up(f.dry.par, rows.dry.data() + b0, R)(f.dry.brk, &rows.brk, 1);
        // dry_rows leaves its scratch zero; a freshly allocated group, or one a failed call left behind, does not hold zeros yet
        WRK_HIP(ctx, hipMemsetAsync(f.dry.scratch, 0, (size_t)R * V * 4, ctx->stream));
    }
    if (up.rc != WRK_OK) return up.rc;
    WRK_HIP(ctx, hipMemsetAsync(io.counter, 0, 4, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// ------------------------------------------------------------------ stop tokens (wrk_stop.hip)
// after wrk_decode_prepare and before the step program is looked up (growing the buffers drops the programs): stop buffers of
// the frame, the B rows, zero just_ended, live = B
// seq (a call with stop sequences, else nullptr): also their buffers, rows and tails [b0, b0 + B) of the pack, match words NONE
static int32_t wrk_stop_prepare(wrk_frame_common& f, const wrk_v7_state* st, uint32_t b0, uint32_t B, const wrk::StopParam* rows,
                                const wrk_stopseq_pack* seq) {
    wrk_ctx* ctx = f.ctx;
    int32_t rc = f.grow(f.stop, {B, (size_t)st->num_layer * (st->head_size + 2) * st->num_emb, f.facts().num_vocab});
    if (rc == WRK_OK && seq) rc = f.grow(f.stop_seq, {B});
    if (rc != WRK_OK) return rc;
    std::vector<uint32_t> flags(f.stop.cap + 1, 0u);      // just_ended = 0, then the live count
    flags[f.stop.cap] = B;
    wrk_upload up{ctx};
    up(f.stop.par, rows, B)(f.stop.flags, flags.data(), flags.size());
    if (seq) {
        const std::vector<uint32_t> none(B, WRK_STOP_MATCH_NONE);
        up(f.stop_seq.rows, seq->rows.data() + b0, B)(f.stop_seq.tail, seq->tails.data() + (size_t)b0 * WRK_STOP_TAIL_LEN, (size_t)B * WRK_STOP_TAIL_LEN);
        up(f.stop_seq.match, none.data(), B);
    }
    if (up.rc != WRK_OK) return up.rc;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// ------------------------------------------------------------------ request queue (wrk_queue.hip)
static int32_t queue_csr_check(wrk_ctx* ctx, const uint32_t* off, uint32_t R, const char* what) {
    WRK_ARG(ctx, off[0] == 0, "%s[0] = %u: must be 0", what, off[0]);
    for (uint32_t r = 0; r < R; ++r) WRK_ARG(ctx, off[r + 1] >= off[r], "%s[%u] = %u decreases", what, r + 1, off[r + 1]);
    return WRK_OK;
}

// generate_queue: the options validated (WRK_E_ARG before any launch) into the request table, the prompt pool and what a request
// carries per feature [R] (wrk_queue_check, wrk_queue_pool_check), then what the B slots start with (wrk_queue_start)
struct wrk_queue_pack {
    uint32_t R = 0, max_steps = 0, poll_steps = 0;
    wrk_step_kind kind{wrk_step_kind::GREEDY, false, wrk_step_kind::QUEUE};       // wrk_queue_pool_check: QUEUE_POOL
    std::vector<wrk::QueueReq> reqs; std::vector<uint32_t> pool;
    // wrk_queue_start, all [B]: the tokens of step 0, the features' rows, the slot records, tails and intake flags; the log [R]; the
    // turnover list of "step -1", the nstart slots that start a request and save nothing; wipe: the leading slots whose window to empty
    std::vector<uint32_t> first_tokens, tails, take;
    wrk_pick_params rows;
    std::vector<wrk::QueueSlot> slots; std::vector<wrk::QueueLog> log; std::vector<wrk::QueueTurn> turn;
    uint32_t nstart = 0, wipe = 0;
    const float* init_state = nullptr;
    // with a state pool; start / save: [R] entries, QUEUE_NO_ENTRY for none
    float* pool_states = nullptr;
    uint32_t pool_entries = 0;
    std::vector<uint32_t> start, save;
    uint32_t* saved_out = nullptr;
    wrk_logprob_call lp;        // the options' log-prob arrays and num_top
    std::vector<float> mu;      // Mirostat / typical: [R] the mu every request starts from
    float* mu_out = nullptr;    // Mirostat: the options' mirostat_mu, or nullptr
    std::vector<uint32_t> gram; // constrained: [R] the automaton state every request starts in
    uint32_t* gram_out = nullptr;   // the options' grammar_state, or nullptr
    std::vector<uint32_t> bias; // biased: [R] the requests' set words
    std::vector<wrk::DryParam> dry; // DRY: [R] the requests' rows (values and tables; a slot's row keeps its own window pointers)
    wrk_token_window* window = nullptr;
    wrk_stopseq_pack seq;      // stop sequences: [R] the requests' rows (the tails: every slot starts empty)
    uint32_t* match_out = nullptr;  // the options' out_stop_match, or nullptr
    std::vector<uint32_t> from;     // prompt intake: [R] the options' prompt_context_from
    const wrk_history_pool* history = nullptr;  // with a state pool: its history pool, or nullptr
    // a guided queue (kind.guided; wrk_queue_guide_check): [R] the negative prompts -- offsets into `pool`, where they follow
    // the prompts, and lengths -- and the scales; the partner halves' start state.  wrk_queue_start: first_tokens, slots and `started`
    // are [2B], pair b the entries b and B + b; pair_started [B]; rows.guide the pairs' scale row [B]
    std::vector<uint32_t> neg_off, neg_len, started, pair_started;
    std::vector<float> scale;
    const float* negative_init_state = nullptr;
};

// guided: the call is wrk_v*_generate_queue_guided's -- B pairs of state slots; the guidance itself: wrk_queue_guide_check, behind this
static int32_t wrk_queue_check(wrk_ctx* ctx, const wrk_queue_options* opt, const wrk_v7_state* st, uint32_t B, uint32_t V, uint32_t mode_arg,
                               wrk_queue_result* out, wrk_queue_pack& pk, bool guided, const wrk_queue_cuts* cuts) {
    WRK_ARG(ctx, opt, "options required");
    WRK_ARG(ctx, out && out->lengths && out->reasons && out->slots && out->start_steps && out->out_tokens && out->steps_run,
            "every result array is required");
    const uint32_t R = opt->num_requests;
    WRK_ARG(ctx, R >= 1, "num_requests 0");
    WRK_ARG(ctx, opt->prompt_tokens && opt->prompt_offsets && opt->max_new, "prompt_tokens, prompt_offsets and max_new are required");
    WRK_ARG(ctx, opt->max_steps >= 1, "max_steps 0");
    pk.lp = wrk_logprob_call{opt->num_top, opt->out_logprob, opt->out_top_ids, opt->out_top_logprobs};
    if (guided) {
        WRK_ARG(ctx, B >= 1 && B <= 128, "num_batch %u: a guided queue has 1 to 128 request slots", B);
        WRK_ARG(ctx, (uint64_t)2 * B <= st->num_batch, "a guided queue of %u request slots needs %u state slots, the state has %u", B, 2 * B, st->num_batch);
    } else {
        WRK_ARG(ctx, B >= 1 && B <= st->num_batch && B <= 256, "num_batch %u: must be in [1, min(%u, 256)]", B, st->num_batch);
    }
    if (((mode_arg >> 8) & 0xffu) > 1)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "generate_queue on several lanes: one queue shared by several streams would need cross-stream atomics");
    WRK_ARG(ctx, !guided || !opt->guidance_scale, "guidance_scale in the options of a guided queue: the scales come from wrk_queue_guidance");
    if (opt->guidance_scale)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "generate_queue with guidance_scale: the negative prompts go through wrk_v*_generate_queue_guided");
    int32_t rc = queue_csr_check(ctx, opt->prompt_offsets, R, "prompt_offsets");
    // the stop sets and the pick parameters go through the validation of the other loops, R rows at a time; of the penalty rows only
    // (presence, frequency, decay) are kept, a slot's row pointers are its own
    std::vector<wrk::StopParam> stops;
    wrk_pick_params req;
    if (rc == WRK_OK) rc = wrk_stop_sets(ctx, opt->stop_tokens, opt->stop_offsets, R, V, "request", stops);
    if (rc == WRK_OK)
        rc = wrk_stop_seqs(ctx, opt->stop_seq_tokens, opt->stop_seq_offsets, opt->stop_seq_owners, opt->out_stop_match != nullptr, nullptr, R, V, "request", pk.seq);
    if (rc == WRK_OK) {
        wrk_pick_args pick = wrk_pick_of(*opt);
        pick.cut = wrk_cut_of(cuts);
        rc = wrk_pick_pack(ctx, pick, R, B, V, req, pk.kind);
    }
    if (rc == WRK_OK) rc = wrk_logprob_check(ctx, pk.lp, V, pk.kind);
    if (rc != WRK_OK) return rc;
    pk.kind.stop_seqs = pk.seq.on;
    pk.match_out = opt->out_stop_match;
    WRK_ARG(ctx, !opt->prompt_context_from || pk.kind.penalized || pk.kind.dry, "prompt_context_from needs an occurrence table or a token window");
    pk.kind.intake = opt->prompt_context_from != nullptr;
    if (pk.kind.intake) pk.from.assign(opt->prompt_context_from, opt->prompt_context_from + R);
    const wrk_step_kind kind = pk.kind;
    pk.R = R; pk.max_steps = opt->max_steps; pk.poll_steps = opt->poll_steps;
    pk.reqs.assign(R, wrk::QueueReq{});
    pk.pool.assign(opt->prompt_tokens, opt->prompt_tokens + opt->prompt_offsets[R]);
    for (size_t i = 0; i < pk.pool.size(); ++i) WRK_ARG(ctx, pk.pool[i] < V, "prompt token %zu: id %u >= vocab %u", i, pk.pool[i], V);
    for (uint32_t r = 0; r < R; ++r) {
        wrk::QueueReq& q = pk.reqs[r];
        q.prompt_off = opt->prompt_offsets[r];
        q.prompt_len = opt->prompt_offsets[r + 1] - opt->prompt_offsets[r];
        WRK_ARG(ctx, q.prompt_len >= 1, "request %u: empty prompt", r);
        q.max_new = opt->max_new[r];
        WRK_ARG(ctx, q.max_new >= 1, "request %u: max_new 0", r);
        if (kind.sampled()) { q.temperature = req.par[r].temperature; q.top_p = req.par[r].top_p; q.seed = req.par[r].seed; }
        q.ln_min_p = -INFINITY;
        if (kind.filtered()) { q.top_k = req.filt[r].top_k; q.ln_min_p = req.filt[r].ln_min_p; }
        q.ln_epsilon = q.ln_eta = -INFINITY;
        if (kind.cut()) {
            const wrk::SampleCut& c = req.cut[r];
            q.top_n_sigma = c.top_n_sigma; q.ln_epsilon = c.ln_epsilon; q.ln_eta = c.ln_eta;
            q.xtc_probability = c.xtc_probability; q.ln_xtc_threshold = c.ln_xtc_threshold;
        }
        q.typical_p = 1.0f;
        if (kind.alt()) { q.tau = req.alt[r].tau; q.eta = req.alt[r].eta; q.typical_p = req.alt[r].typical_p; }
        if (kind.penalized) { q.presence = req.pen[r].presence; q.frequency = req.pen[r].frequency; q.decay = req.pen[r].decay; }
        q.stop_count = stops[r].count;
        memcpy(q.stop_ids, stops[r].ids, sizeof q.stop_ids);
    }
    if (opt->init_state) {
        const size_t need = (size_t)st->num_layer * (st->head_size + 2) * st->num_emb * 4;
        WRK_ARG(ctx, opt->init_state->ctx == ctx, "init_state belongs to another context");
        WRK_ARG(ctx, opt->init_state->bytes == need, "init_state holds %zu bytes, a sequence's state is %zu", opt->init_state->bytes, need);
        pk.init_state = (const float*)opt->init_state->ptr;
    }
    // what a request carries besides its QueueReq
    for (uint32_t r = 0; r < R && kind.alt(); ++r) pk.mu.push_back(req.alt[r].mu);
    pk.mu_out = kind.mirostat() ? opt->mirostat_mu : nullptr;
    if (kind.constrained) { pk.gram = req.gram_state; pk.gram_out = opt->grammar_state; pk.rows.grammar = req.grammar; }
    if (kind.biased) { pk.bias = req.bias_set; pk.rows.bias = req.bias; }
    if (kind.dry) { pk.dry = req.dry; pk.window = opt->window; pk.rows.has_dry = true; pk.rows.brk = req.brk; }
    return WRK_OK;
}

// after wrk_queue_check: the pool of wrk_v*_generate_queue_pool validated into pk (WRK_E_ARG / WRK_E_UNSUPPORTED before any launch)
static int32_t wrk_queue_pool_check(wrk_ctx* ctx, const wrk_queue_pool* pool, const wrk_queue_options* opt, const wrk_v7_state* st, uint32_t V,
                                    wrk_queue_pack& pk) {
    WRK_ARG(ctx, pool, "pool required");
    WRK_ARG(ctx, pool->states, "%s", pool->start || pool->save ? "start / save entries without a pool buffer" : "the pool has no buffer");
    const uint32_t R = pk.R, P = pool->num_entries;
    const size_t slot = (size_t)(st->head_size + 2) * st->num_emb, one = (size_t)st->num_layer * slot * 4;
    WRK_ARG(ctx, pool->states->ctx == ctx, "the pool belongs to another context");
    WRK_ARG(ctx, P >= 1 && pool->states->bytes / one == P && pool->states->bytes % one == 0,
            "the pool holds %zu bytes: not %u entries of %zu", pool->states->bytes, P, one);
    WRK_ARG(ctx, !opt->init_state || (opt->init_state != pool->states && opt->init_state->ptr != pool->states->ptr),
            "the pool and init_state are one buffer");
    pk.start.assign(R, wrk::QUEUE_NO_ENTRY);
    pk.save.assign(R, wrk::QUEUE_NO_ENTRY);
    std::vector<uint32_t> saver(P, wrk::QUEUE_NO_ENTRY);       // the request that saves to the entry
    for (uint32_t r = 0; r < R; ++r) {
        if (pool->start) pk.start[r] = pool->start[r];
        if (pool->save) pk.save[r] = pool->save[r];
        WRK_ARG(ctx, pk.start[r] == wrk::QUEUE_NO_ENTRY || pk.start[r] < P, "request %u: start entry %u of %u", r, pk.start[r], P);
        const uint32_t k = pk.save[r];
        if (k == wrk::QUEUE_NO_ENTRY) continue;
        WRK_ARG(ctx, k < P, "request %u: save entry %u of %u", r, k, P);
        WRK_ARG(ctx, saver[k] == wrk::QUEUE_NO_ENTRY, "requests %u and %u both save to entry %u", saver[k], r, k);
        saver[k] = r;
    }
    // a request may read the entry it saves to itself (the read at its start precedes the write at its end); another request's
    // target would make the result depend on the schedule
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t k = pk.start[r];
        WRK_ARG(ctx, k == wrk::QUEUE_NO_ENTRY || saver[k] == wrk::QUEUE_NO_ENTRY || saver[k] == r,
                "request %u starts from entry %u, which request %u saves to", r, k, k == wrk::QUEUE_NO_ENTRY ? 0u : saver[k]);
    }
    if (const wrk_history_pool* hp = opt->history) {
        WRK_ARG(ctx, pk.kind.penalized || pk.kind.dry, "a history pool needs an occurrence table or a token window");
        WRK_ARG(ctx, hp->ctx == ctx, "the history pool belongs to another context");
        WRK_ARG(ctx, hp->num_vocab == V, "history pool of %u tokens, logits of %u", hp->num_vocab, V);
        WRK_ARG(ctx, hp->num_entries == P, "history pool of %u entries, state pool of %u", hp->num_entries, P);
        WRK_ARG(ctx, !pk.kind.dry || hp->capacity != 0, "a token window with a history pool created without windows");
        WRK_ARG(ctx, pk.kind.dry || hp->capacity == 0, "a history pool with windows and no token window");
        WRK_ARG(ctx, !pk.kind.dry || hp->capacity == opt->window->capacity, "history pool windows of capacity %u, token window of %u",
                hp->capacity, opt->window->capacity);
        pk.history = hp;
        pk.kind.history = true;
    }
    if (slot % 4 != 0) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "a state pool needs (S + 2) * D = %zu to be a multiple of 4", slot);
    if ((((uintptr_t)pool->states->ptr) | ((uintptr_t)st->data) | ((uintptr_t)pk.init_state)) & 15u)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "a state pool needs 16-byte aligned state, pool and init_state buffers");
    pk.kind.tail = wrk_step_kind::QUEUE_POOL;
    pk.pool_states = (float*)pool->states->ptr;
    pk.pool_entries = P;
    pk.saved_out = pool->saved;
    return WRK_OK;
}

// after wrk_queue_check(guided): the guidance of wrk_v*_generate_queue_guided validated into pk (WRK_E_ARG / WRK_E_UNSUPPORTED before any
// launch): the scales, the negative prompts appended to the token pool, the partners' start state; sets kind.guided
static int32_t wrk_queue_guide_check(wrk_ctx* ctx, const wrk_queue_guidance* guide, const wrk_queue_options* opt, const wrk_v7_state* st, uint32_t V,
                                     wrk_queue_pack& pk) {
    WRK_ARG(ctx, guide, "guide required");
    WRK_ARG(ctx, guide->scale && guide->negative_offsets, "scale and negative_offsets are required");
    const uint32_t R = pk.R;
    int32_t rc = wrk_guide_pack(ctx, guide->scale, R, V, pk.scale);
    if (rc == WRK_OK) rc = queue_csr_check(ctx, guide->negative_offsets, R, "negative_offsets");
    if (rc != WRK_OK) return rc;
    WRK_ARG(ctx, guide->negative_tokens || guide->negative_offsets[R] == 0, "negative_offsets name %u tokens, negative_tokens is NULL",
            guide->negative_offsets[R]);
    const uint32_t base = (uint32_t)pk.pool.size();
    for (uint32_t i = 0; i < guide->negative_offsets[R]; ++i) {
        WRK_ARG(ctx, guide->negative_tokens[i] < V, "negative token %u: id %u >= vocab %u", i, guide->negative_tokens[i], V);
        pk.pool.push_back(guide->negative_tokens[i]);
    }
    for (uint32_t r = 0; r < R; ++r) {
        pk.neg_off.push_back(base + guide->negative_offsets[r]);
        pk.neg_len.push_back(guide->negative_offsets[r + 1] - guide->negative_offsets[r]);
        WRK_ARG(ctx, pk.neg_len[r] != 0 || pk.scale[r] == 1.0f, "request %u: an empty negative prompt with guidance scale %g (only 1 runs without a partner)",
                r, (double)pk.scale[r]);
    }
    if (const wrk_buf* ns = guide->negative_init_state) {
        const size_t need = (size_t)st->num_layer * (st->head_size + 2) * st->num_emb * 4;
        WRK_ARG(ctx, ns->ctx == ctx, "negative_init_state belongs to another context");
        WRK_ARG(ctx, ns->bytes == need, "negative_init_state holds %zu bytes, a sequence's state is %zu", ns->bytes, need);
        WRK_ARG(ctx, !opt->init_state || (ns != opt->init_state && ns->ptr != opt->init_state->ptr), "init_state and negative_init_state are one buffer");
        pk.negative_init_state = (const float*)ns->ptr;
    }
    pk.kind.guided = true;
    return WRK_OK;
}

static wrk::QueueBufs queue_bufs(const wrk_frame_common& f, wrk_step_kind kind) {
    if (kind.guided) {
        wrk_step_kind plain = kind;
        plain.guided = false;
        wrk::QueueBufs q = queue_bufs(f, plain);
        q.neg_off = f.queue_guide.neg_off; q.neg_len = f.queue_guide.neg_len; q.scale_req = f.queue_guide.scale; q.scale = f.guide.par;
        q.pair_started = f.queue_guide.pair_started;
        return q;
    }
    if (kind.cut()) {
        wrk_step_kind filt = kind;
        filt.pick = wrk_step_kind::FILTERED;
        wrk::QueueBufs q = queue_bufs(f, filt);
        q.cut_par = f.cut_par.par;
        return q;
    }
    return wrk::QueueBufs{f.queue.slots, f.queue.reqs, f.queue.pool, f.queue.log, f.queue.ctl, f.queue.started,
                          kind.sampled() ? f.sample.par : nullptr, kind.penalized ? f.penalty.par : nullptr, kind.filtered() ? f.filter.par : nullptr,
                          kind.alt() ? f.alt.par : nullptr, kind.mirostat() ? f.queue.mu : nullptr,
                          kind.constrained ? f.grammar.state : nullptr, kind.constrained ? f.queue.gram : nullptr,
                          kind.dry ? f.dry.par : nullptr, kind.dry ? f.queue.dry : nullptr,
                          kind.stop_seqs ? f.queue.seq_rows : nullptr, kind.stop_seqs ? f.queue_seq.tail : nullptr,
                          kind.stop_seqs ? f.queue.seq_match : nullptr,
                          kind.intake ? f.queue.from : nullptr, kind.intake ? f.queue_intake.flags : nullptr,
                          kind.biased ? f.bias.set : nullptr, kind.biased ? f.queue.bias : nullptr};
}

static wrk::QueueStateBufs queue_state_bufs(const wrk_frame_common& f, wrk_step_kind kind) {
    return wrk::QueueStateBufs{f.queue.start, f.queue.save, f.queue_states.ctl, f.queue_states.turn, kind.history};
}

// The host's step 0, after the checks.  Every slot gets valid rows, which an idle slot (b >= R) keeps -- a valid token, state 0, which
// every grammar has, no bias set -- with the pointers that are the slot's whatever request it serves: row b of the occurrence table, slot b of the
// window.  Then the dispatch rule deals request b to slot b < min(B, R) with first_step 0, over host mirrors of the device's arrays
static void wrk_queue_start(const wrk_queue_options* opt, uint32_t B, wrk_queue_pack& pk) {
    const wrk_step_kind kind = pk.kind;
    wrk_pick_params& rows = pk.rows;
    const uint32_t FB = kind.guided ? 2 * B : B;        // a guided queue: B pairs, the rows below B wide, the records and tokens 2B
    pk.first_tokens.assign(FB, pk.pool[0]);
    if (kind.guided) rows.guide.assign(B, 1.0f);
    if (kind.sampled()) rows.par.assign(B, wrk::SampleParam{1.0f, 0.0f, 0u, 0u});
    if (kind.filtered()) rows.filt.assign(B, wrk::SampleFilter{0u, -INFINITY});
    if (kind.alt()) rows.alt.assign(B, wrk::SampleAlt{0.0f, 0.0f, 0.0f, 1.0f});
    if (kind.cut()) rows.cut.assign(B, wrk::SampleCut{0.0f, -INFINITY, -INFINITY, 0.0f, 0.0f});
    if (kind.constrained) rows.gram_state.assign(B, 0u);
    if (kind.biased) rows.bias_set.assign(B, WRK_BIAS_NONE);
    for (uint32_t b = 0; b < B && kind.penalized; ++b) rows.pen.push_back(opt->occ->row(b, 0.0f, 0.0f, 1.0f));
    for (uint32_t b = 0; b < B && kind.dry; ++b) {
        rows.dry.push_back(pk.dry[0]);
        rows.dry[b].ring = pk.window->ring + (size_t)b * pk.window->capacity;
        rows.dry[b].meta = pk.window->meta + (size_t)b * 2;
    }
    pk.slots.assign(FB, wrk::QueueSlot{0u, 0u, 0u, wrk::QUEUE_IDLE});
    pk.log.assign(pk.R, wrk::QueueLog{0u, 0u, 0u, 0u});
    if (kind.stop_seqs) pk.tails.assign((size_t)B * WRK_STOP_TAIL_LEN, WRK_STOP_TAIL_EMPTY);
    if (kind.intake) pk.take.assign(B, 0u);
    pk.nstart = B < pk.R ? B : pk.R;
    pk.turn.resize(pk.nstart);
    // as queue_bufs: an array is nullptr exactly when the kind is without its feature (a vector of the pack is empty then)
    auto at = [](auto& v) { return v.empty() ? nullptr : v.data(); };
    wrk::QueueBufs Q{pk.slots.data(), pk.reqs.data(), pk.pool.data(), pk.log.data(), nullptr, nullptr, at(rows.par), at(rows.pen), at(rows.filt),
                     at(rows.alt), kind.mirostat() ? pk.mu.data() : nullptr, at(rows.gram_state), at(pk.gram), at(rows.dry), at(pk.dry),
                     at(pk.seq.rows), at(pk.tails), nullptr, at(pk.from), at(pk.take), at(rows.bias_set), at(pk.bias)};
    Q.cut_par = at(rows.cut);
    const wrk::QueueStateBufs P{pk.start.data(), pk.save.data(), nullptr, pk.turn.data(), kind.history};
    if (kind.guided) {
        // the guided rule over the same mirrors: a half's start flag is raised when it feeds its first token at step 0, the others wait
        wrk::QueueBufs G = Q;
        G.neg_off = pk.neg_off.data(); G.neg_len = pk.neg_len.data(); G.scale_req = pk.scale.data(); G.scale = rows.guide.data();
        pk.started.assign(FB, 0u);
        pk.pair_started.assign(B, 0u);
        for (uint32_t b = 0; b < pk.nstart; ++b) {
            const wrk::QueuePairStart ps = wrk::queue_dispatch_guided(G, pk.first_tokens.data(), b, b, B, 0u);
            if (ps.wipe) pk.wipe = b + 1;
            pk.started[b] = ps.start_cond; pk.started[B + b] = ps.start_part; pk.pair_started[b] = 1u;
        }
        return;
    }
    for (uint32_t b = 0; b < pk.nstart; ++b)
        if (wrk::queue_dispatch(Q, pk.first_tokens.data(), b, b, 0u, kind.pool() ? &P : nullptr, b)) pk.wipe = b + 1;
}

static wrk::QueueGeom queue_geom(const wrk_v7_state* st, uint32_t b0, uint32_t V) {
    return wrk::QueueGeom{st->data, st->num_layer, st->num_batch, b0, V, (size_t)(st->head_size + 2) * st->num_emb};
}

// prompt intake (intake kinds): the prompt tokens that advance_queue -- or, for step 0, the host -- marked in the intake flags enter
// the slots' occurrence rows (penalised) and windows (dry) from io.tokens, with the launches that take a counted draw in
static int32_t enqueue_prompt_intake(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, hipStream_t q) {
    if (!kind.intake) return WRK_OK;
    if (!f.queue_intake.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "intake buffers are not prepared");
    if (kind.dry && !f.dry.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "DRY rows are not prepared");
    const wrk::RowGate gate{f.queue_intake.flags, 1u, 1u};
    const uint32_t V = f.facts().num_vocab;
    if (kind.penalized) wrk::occurrence_update(q, V, B, f.penalty.par, f.io().tokens, 1, gate);
    if (kind.dry) wrk::window_push(q, V, B, f.dry.par, f.io().tokens, gate);
    return WRK_OK;
}

// after wrk_decode_prepare, which uploaded the slots' tokens and rows of step 0, and before the step program is looked up (growing the
// buffers drops the programs): the queue's buffers grown, the tables and what wrk_queue_start left for the slots uploaded, live = R;
// then queue_reset of the slots that start at step 0 on the submission stream (with a pool: queue_turnover on the list of those slots)
// A guided queue: FB = 2B sequences of the lane -- the slot records and start flags are FB wide, everything else B -- and
// queue_reset_guided resets the halves that start at step 0
static int32_t wrk_queue_prepare(wrk_frame_common& f, const wrk_v7_state* st, uint32_t FB, const wrk_queue_pack& pk) {
    wrk_ctx* ctx = f.ctx;
    const uint32_t V = f.facts().num_vocab;
    const wrk_step_kind kind = pk.kind;
    const uint32_t B = kind.guided ? FB / 2 : FB;
    // never smaller than before: a later, smaller queue reuses the buffers and the program
    int32_t rc = f.grow(f.queue, {FB, pk.R, pk.pool.size()});
    if (rc == WRK_OK && pk.kind.pool()) rc = f.grow(f.queue_states, {B});
    if (rc == WRK_OK && pk.kind.stop_seqs) rc = f.grow(f.queue_seq, {B});
    if (rc == WRK_OK && pk.kind.intake) rc = f.grow(f.queue_intake, {B});
    if (rc == WRK_OK && kind.guided) rc = f.grow(f.queue_guide, {B, pk.R});
    if (rc != WRK_OK) return rc;
    std::vector<uint32_t> started(FB, 0u);
    for (uint32_t b = 0; b < pk.nstart; ++b) started[b] = 1u;
    if (kind.guided) started = pk.started;
    const wrk::QueueCtl ctl{pk.nstart, pk.R, pk.R, 0u, pk.init_state, pk.negative_init_state};
    wrk_upload up{ctx};
    up(f.queue.slots, pk.slots.data(), FB)(f.queue.started, started.data(), FB)(f.queue.log, pk.log.data(), pk.R)(f.queue.reqs, pk.reqs.data(), pk.R);
    up(f.queue.pool, pk.pool.data(), pk.pool.size())(f.queue.ctl, &ctl, 1);
    if (kind.guided) {
        up(f.queue_guide.pair_started, pk.pair_started.data(), B)(f.queue_guide.neg_off, pk.neg_off.data(), pk.R);
        up(f.queue_guide.neg_len, pk.neg_len.data(), pk.R)(f.queue_guide.scale, pk.scale.data(), pk.R);
    }
    if (kind.mirostat()) up(f.queue.mu, pk.mu.data(), pk.R);
    if (kind.constrained) up(f.queue.gram, pk.gram.data(), pk.R);
    if (kind.biased) up(f.queue.bias, pk.bias.data(), pk.R);
    if (kind.dry) up(f.queue.dry, pk.dry.data(), pk.R);
    // a slot that starts a request at step 0 begins with an empty window, as a refilled slot does
    const std::vector<uint32_t> empty((size_t)pk.wipe * 2, 0u);
    if (pk.wipe) up(pk.window->meta, empty.data(), empty.size());
    if (kind.stop_seqs) {       // no request has a match yet
        const std::vector<uint32_t> none(pk.R, WRK_STOP_MATCH_NONE);
        up(f.queue.seq_rows, pk.seq.rows.data(), pk.R)(f.queue_seq.tail, pk.tails.data(), pk.tails.size())(f.queue.seq_match, none.data(), pk.R);
    }
    if (kind.pool()) {
        const wrk::QueueStateCtl sctl{pk.pool_states, pk.pool_entries, pk.nstart, pk.history ? pk.history->dev() : wrk::QueueHistory{}};
        up(f.queue.start, pk.start.data(), pk.R)(f.queue.save, pk.save.data(), pk.R);
        up(f.queue_states.turn, pk.turn.data(), pk.nstart)(f.queue_states.ctl, &sctl, 1);
    }
    if (kind.intake) up(f.queue_intake.flags, pk.take.data(), B)(f.queue.from, pk.from.data(), pk.R);
    if (up.rc != WRK_OK) return up.rc;
    // the slots that start a request at step 0 are reset as the step that ends a request resets its slot
    if (pk.kind.pool()) wrk::queue_turnover(ctx->stream, queue_geom(st, 0, V), queue_bufs(f, pk.kind), queue_state_bufs(f, kind), B, ctx->num_cu);
    else if (kind.guided) wrk::queue_reset_guided(ctx->stream, queue_geom(st, 0, V), queue_bufs(f, pk.kind), B, ctx->num_cu);
    else wrk::queue_reset(ctx->stream, queue_geom(st, 0, V), queue_bufs(f, pk.kind), B, ctx->num_cu);
    // and takes its intake as a step's tail does: the first tokens are in io.tokens (wrk_decode_prepare)
    const int32_t irc = enqueue_prompt_intake(f, B, pk.kind, ctx->stream);
    if (irc != WRK_OK) return irc;
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// Whether a row's draw of this step counts -- moves its Mirostat mu, enters its occurrence row -- as one RowGate for both: the flag the
// previous step's advance wrote.  A finished sequence of a stop program, a prompt-phase or an idle slot of a queue program does not count
static int32_t draw_gate(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, wrk::RowGate& g) {
    g = wrk::RowGate{nullptr, 0u, 0u};
    if (kind.tail == wrk_step_kind::STOP) {
        if (!f.stop.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "stop buffers are not prepared");
        g = wrk::RowGate{&f.stop.par->done, sizeof(wrk::StopParam) / 4, 0u};
    } else if (kind.queue()) {
        if (!f.queue.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "queue buffers are not prepared");
        g = wrk::RowGate{&f.queue.slots->phase, sizeof(wrk::QueueSlot) / 4, wrk::QUEUE_REPLY};
    }
    return WRK_OK;
}

// the occurrence rows count the drawn tokens in io.argmax (penalised kinds), under the step's gate
static int32_t enqueue_occurrence_update(wrk_frame_common& f, uint32_t B, wrk_step_kind kind) {
    if (!kind.penalized) return WRK_OK;
    wrk::RowGate gate;
    const int32_t rc = draw_gate(f, B, kind, gate);
    if (rc != WRK_OK) return rc;
    wrk::occurrence_update(f.ctx->op_stream(), f.facts().num_vocab, B, f.penalty.par, f.io().argmax, 1, gate);
    return WRK_OK;
}

// the automaton states move on the drawn tokens in io.argmax (constrained kinds), under the step's gate
static int32_t enqueue_grammar_advance(wrk_frame_common& f, uint32_t B, wrk_step_kind kind) {
    if (!kind.constrained) return WRK_OK;
    if (!f.grammar.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "grammar states are not prepared");
    wrk::RowGate gate;
    const int32_t rc = draw_gate(f, B, kind, gate);
    if (rc != WRK_OK) return rc;
    wrk::grammar_advance(f.ctx->op_stream(), f.facts().num_vocab, B, f.grammar.par, f.io().argmax, gate);
    return WRK_OK;
}

// the token windows take the drawn tokens in io.argmax (DRY kinds), under the step's gate
static int32_t enqueue_window_push(wrk_frame_common& f, uint32_t B, wrk_step_kind kind) {
    if (!kind.dry) return WRK_OK;
    if (!f.dry.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "DRY rows are not prepared");
    wrk::RowGate gate;
    const int32_t rc = draw_gate(f, B, kind, gate);
    if (rc != WRK_OK) return rc;
    wrk::window_push(f.ctx->op_stream(), f.facts().num_vocab, B, f.dry.par, f.io().argmax, gate);
    return WRK_OK;
}

// what a tail does with the drawn tokens before it advances: the occurrence update, then the automaton advance, then the window push
static int32_t enqueue_draw_updates(wrk_frame_common& f, uint32_t B, wrk_step_kind kind) {
    int32_t rc = enqueue_occurrence_update(f, B, kind);
    if (rc == WRK_OK) rc = enqueue_grammar_advance(f, B, kind);
    return rc == WRK_OK ? enqueue_window_push(f, B, kind) : rc;
}

// a guided step, behind the draw updates of its R conditional sequences and in front of the advance: the partners take the same tokens
static void enqueue_guide_follow(wrk_frame_common& f, uint32_t R, wrk_step_kind kind) {
    if (kind.guided) wrk::guide_follow(f.ctx->op_stream(), f.io().argmax, R);
}

// tail of a queue program's step, after io.argmax holds the drawn tokens: the occurrence update of the slots whose draw is a reply
// token (penalised), advance_queue, queue_reset of slots [b0, b0 + B) of `st`; with a pool advance_queue_pool and queue_turnover,
// launch for launch; a guided queue (B pairs): guide_follow, advance_queue_guided, queue_reset_guided over 2B slots
static int32_t enqueue_queue_tail(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, const wrk_v7_state* st, uint32_t b0) {
    hipStream_t q = f.ctx->op_stream();
    const wrk::FrameIo& io = f.io();
    const uint32_t V = f.facts().num_vocab;
    const uint32_t FB = kind.guided ? 2 * B : B;        // a guided queue: B pairs of slots
    if (!f.queue.holds({FB}) || b0 != 0 || FB > st->num_batch) return wrk_fail(f.ctx, WRK_E_ARG, "queue buffers are not prepared");
    if (kind.guided && (kind.pool() || B > 128 || !f.queue_guide.holds({B}) || !f.guide.holds({B})))
        return wrk_fail(f.ctx, WRK_E_ARG, "guided queue buffers are not prepared");
    if (kind.stop_seqs && !f.queue_seq.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "stop-sequence buffers are not prepared");
    if (kind.pool() && (!f.queue_states.holds({B}) || ((size_t)(st->head_size + 2) * st->num_emb) % 4 != 0))
        return wrk_fail(f.ctx, WRK_E_ARG, "state pool buffers are not prepared");
    const int32_t rc = enqueue_draw_updates(f, B, kind);
    if (rc != WRK_OK) return rc;
    const wrk::QueueBufs bufs = queue_bufs(f, kind);
    if (kind.guided) {
        // the partners take the conditional halves' draws, then the pairs advance and the halves that start are reset
        enqueue_guide_follow(f, B, kind);
        wrk::advance_queue_guided(q, io.argmax, io.tokens, f.history.tokens, io.counter, bufs, B);
        wrk::queue_reset_guided(q, queue_geom(st, b0, V), bufs, B, f.ctx->num_cu);
    } else if (kind.pool()) {
        wrk::advance_queue_pool(q, io.argmax, io.tokens, f.history.tokens, io.counter, bufs, queue_state_bufs(f, kind), B);
        wrk::queue_turnover(q, queue_geom(st, b0, V), bufs, queue_state_bufs(f, kind), B, f.ctx->num_cu);
    } else {
        wrk::advance_queue(q, io.argmax, io.tokens, f.history.tokens, io.counter, bufs, B);
        wrk::queue_reset(q, queue_geom(st, b0, V), bufs, B, f.ctx->num_cu);
    }
    return enqueue_prompt_intake(f, B, kind, q);
}

// after the loop: the log and the history rows (with log-probs: their rows too) come back and the replies are cut out of them
// A guided queue: the history rows are 2B wide and the replies are in columns [0, B); the log-prob rows are B wide
static int32_t wrk_queue_finish(wrk_frame_common& f, uint32_t B, uint32_t steps_run, const wrk_queue_pack& pk, const wrk_queue_options* opt,
                                wrk_queue_result* out) {
    wrk_ctx* ctx = f.ctx;
    const size_t HB = pk.kind.guided ? (size_t)2 * B : B;
    std::vector<wrk::QueueLog> log(pk.R);
    std::vector<uint32_t> hist((size_t)steps_run * HB);
    WRK_HIP(ctx, hipMemcpyAsync(log.data(), f.queue.log, (size_t)pk.R * sizeof(wrk::QueueLog), hipMemcpyDeviceToHost, ctx->stream));
    if (!hist.empty()) WRK_HIP(ctx, hipMemcpyAsync(hist.data(), f.history.tokens, hist.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    const size_t nt = pk.lp.num_top;
    std::vector<float> lp_rows(pk.lp.on() ? (size_t)steps_run * B : 0), top_lp(lp_rows.size() * nt);
    std::vector<uint32_t> top_id(top_lp.size());
    if (!lp_rows.empty()) WRK_HIP(ctx, hipMemcpyAsync(lp_rows.data(), f.logprob.logprob, lp_rows.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (!top_lp.empty()) {
        WRK_HIP(ctx, hipMemcpyAsync(top_id.data(), f.logprob.top_ids, top_id.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(top_lp.data(), f.logprob.top_logprobs, top_lp.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    // Mirostat: a request that ended left its mu in its own entry; one still running (reason 3) has it in its slot's row
    auto final_of = [](const wrk::QueueLog& g, auto in_slot, auto in_entry) { return g.reason == 3 ? in_slot : in_entry; };
    std::vector<float> mu_req(pk.mu_out ? pk.R : 0);
    std::vector<wrk::SampleAlt> mu_slot(pk.mu_out ? B : 0);
    if (pk.mu_out) {
        WRK_HIP(ctx, hipMemcpyAsync(mu_req.data(), f.queue.mu, (size_t)pk.R * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(mu_slot.data(), f.alt.par, (size_t)B * sizeof(wrk::SampleAlt), hipMemcpyDeviceToHost, ctx->stream));
    }
    // constrained: the same two places hold a request's automaton state
    std::vector<uint32_t> gram_req(pk.gram_out ? pk.R : 0), gram_slot(pk.gram_out ? B : 0);
    if (pk.gram_out) {
        WRK_HIP(ctx, hipMemcpyAsync(gram_req.data(), f.queue.gram, (size_t)pk.R * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(gram_slot.data(), f.grammar.state, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    // stop sequences: a request's match word is written by the step that ends it with reason 1, and by nothing else
    std::vector<uint32_t> match(pk.match_out ? pk.R : 0);
    if (pk.match_out) WRK_HIP(ctx, hipMemcpyAsync(match.data(), f.queue.seq_match, (size_t)pk.R * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t o = 0;
    for (uint32_t r = 0; r < pk.R; ++r) {
        wrk::QueueLog g = log[r];
        const wrk::QueueReq& q = pk.reqs[r];
        // dealt to a slot by the last step that ran: its p_0 was never fed, so it was never dispatched
        if (g.reason == 3 && g.start_step >= steps_run) g = wrk::QueueLog{0u, 0u, 0u, 0u};
        // reply token j was drawn by step start_step + n - 1 + j; nothing below can leave the rows that ran unless the device log is wrong
        if (g.length > q.max_new || g.slot >= B || (g.length && (size_t)g.start_step + q.prompt_len - 1 + g.length > steps_run))
            return wrk_fail(ctx, WRK_E_HIP, "request %u: inconsistent queue log (length %u slot %u start %u)", r, g.length, g.slot, g.start_step);
        out->lengths[r] = g.length; out->reasons[r] = g.reason; out->slots[r] = g.slot; out->start_steps[r] = g.start_step;
        if (pk.mu_out && g.reason != 0) pk.mu_out[r] = final_of(g, mu_slot[g.slot].mu, mu_req[r]);
        if (pk.gram_out && g.reason != 0) pk.gram_out[r] = final_of(g, gram_slot[g.slot], gram_req[r]);
        if (pk.match_out) pk.match_out[r] = g.reason == 1 ? match[r] : WRK_STOP_MATCH_NONE;
        // the step that gave the request reason 1 or 2 also wrote its state to its entry (queue_turnover)
        if (pk.saved_out) pk.saved_out[r] = pk.save[r] != wrk::QUEUE_NO_ENTRY && (g.reason == 1 || g.reason == 2);
        for (uint32_t j = 0; j < g.length; ++j) {
            const size_t at = (size_t)g.start_step + q.prompt_len - 1 + j, row = at * B + g.slot;
            out->out_tokens[o + j] = hist[at * HB + g.slot];
            if (!pk.lp.on()) continue;
            pk.lp.logprob[o + j] = lp_rows[row];
            for (size_t t = 0; t < nt; ++t) { pk.lp.top_ids[(o + j) * nt + t] = top_id[row * nt + t]; pk.lp.top_logprobs[(o + j) * nt + t] = top_lp[row * nt + t]; }
        }
        o += opt->max_new[r];
    }
    *out->steps_run = steps_run;
    return WRK_OK;
}

static wrk::StopGeom stop_geom(wrk_frame_common& f, const wrk_v7_state* st, uint32_t b0) {
    const wrk::FrameIo& io = f.io();
    wrk::StopGeom g{};
    g.state = st->data; g.head_o = io.head_o; g.snap_state = f.stop.snap_state; g.snap_logits = f.stop.snap_logits;
    g.just_ended = f.stop.just_ended(); g.par = f.stop.par; g.counter = io.counter; g.lengths = f.stop.lengths();
    g.layers = st->num_layer; g.num_batch = st->num_batch; g.b0 = b0; g.v = f.facts().num_vocab;
    g.slot = (size_t)(st->head_size + 2) * st->num_emb;
    return g;
}

// tail of a stop program's step, after io.argmax holds the drawn tokens: the occurrence update of the sequences still running
// (penalised), advance_stop, stop_snapshot of sequences [b0, b0 + B) of `st`.  R: the rows of the pick (a guided step: B / 2, and
// guide_follow between their draw updates and the advance)
static int32_t enqueue_stop_tail(wrk_frame_common& f, uint32_t B, uint32_t R, wrk_step_kind kind, const wrk_v7_state* st, uint32_t b0) {
    hipStream_t q = f.ctx->op_stream();
    const wrk::FrameIo& io = f.io();
    if (!f.stop.holds({B}) || b0 + B > st->num_batch) return wrk_fail(f.ctx, WRK_E_ARG, "stop buffers are not prepared");
    const int32_t rc = enqueue_draw_updates(f, R, kind);
    if (rc != WRK_OK) return rc;
    enqueue_guide_follow(f, R, kind);
    if (kind.stop_seqs) {
        if (!f.stop_seq.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "stop-sequence buffers are not prepared");
        wrk::advance_stop_seq(q, io.argmax, io.tokens, f.history.tokens, io.counter, f.stop.par, f.stop.just_ended(), f.stop.live(),
                              wrk::StopSeqBufs{f.stop_seq.rows, f.stop_seq.tail, f.stop_seq.match}, B);
    } else {
        wrk::advance_stop(q, io.argmax, io.tokens, f.history.tokens, io.counter, f.stop.par, f.stop.just_ended(), f.stop.live(), B);
    }
    wrk::stop_snapshot(q, stop_geom(f, st, b0), B, f.ctx->num_cu);
    return WRK_OK;
}

// ------------------------------------------------------------------ beam search (wrk_beam.hip)
// generate_beam: the options validated (WRK_E_ARG before any launch) into what the B = G * W slots start with
struct wrk_beam_pack {
    uint32_t G = 0, W = 0, steps = 0, poll_steps = 0;
    std::vector<uint32_t> first_tokens;         // [B]: every slot of group g feeds first_tokens[g]
    std::vector<wrk::BeamSlot> slots;           // [B]: slot gW LIVE with score 0 and length 0, the others DEAD
    std::vector<wrk::BeamStop> stops;           // [G]
    std::vector<float> inv_norm;                // [steps + 1]
    // biased: the object and the slots' set words [B]; with a context the slots' penalty rows, DRY rows and start states [B]
    wrk_pick_params rows;
    size_t ctx_vocab = 0, ctx_capacity = 0;     // what the context scratch is sized by: V with a table, the window's capacity
    uint32_t* out_grammar_state = nullptr;      // [B], or nullptr
    bool context() const { return !rows.pen.empty() || rows.has_dry || rows.grammar; }
};

static size_t state_slot_floats(const wrk_v7_state* st) { return (size_t)(st->head_size + 2) * st->num_emb; }

// after wrk_decode_prepare and before the step program is looked up (growing the buffers drops the programs): the beam buffers of the
// frame, the parameter blocks, the records, the stop sets and inv_norm of this call, empty maps, live = G
static int32_t wrk_beam_prepare(wrk_frame_common& f, const wrk_v7_state* st, uint32_t B, const wrk_beam_pack& pk) {
    wrk_ctx* ctx = f.ctx;
    int32_t rc = f.grow(f.beam, {B, (size_t)pk.steps * B, pk.inv_norm.size(), (size_t)st->num_layer * state_slot_floats(st)});
    if (rc == WRK_OK && pk.context()) rc = f.grow(f.beam_ctx, {B, pk.ctx_vocab, pk.ctx_capacity});
    if (rc != WRK_OK) return rc;
    const wrk::BeamParam par{pk.W, pk.G, pk.steps, (uint32_t)pk.inv_norm.size()};
    const wrk::LogprobParam lp{f.beam.chosen_lp, f.beam.cand_ids, f.beam.cand_lp, pk.W, B};
    const std::vector<uint32_t> none(B, WRK_BEAM_NO_COPY);
    wrk_upload up{ctx};
    up(f.beam.par, &par, 1)(f.beam.lp_par, &lp, 1)(f.beam.slots, pk.slots.data(), B)(f.beam.stops, pk.stops.data(), pk.G);
    up(f.beam.inv_norm, pk.inv_norm.data(), pk.inv_norm.size())(f.beam.copy_src, none.data(), B)(f.beam.snap_map, none.data(), B);
    up(f.beam.done_map, none.data(), B)(f.beam.live, &pk.G, 1);
    if (up.rc != WRK_OK) return up.rc;
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

// the slots [b0, b0 + B) of `st`, as beam_copy addresses them
static wrk::BeamSlots beam_state(const wrk_v7_state* st, uint32_t b0) { return wrk::BeamSlots{st->data, st->num_batch, b0}; }

// The context stages of a pick's row chain, behind the bias and in front of the pick or the beam front: the penalise launch (penalised),
// the DRY launches (dry: the row copy unless penalised, then dry_rows) and the mask launch (constrained).  `logits`: the row the chain
// has reached, in and out
static int32_t enqueue_context_rows(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, const float*& logits, bool argmax_done) {
    hipStream_t q = f.ctx->op_stream();
    const uint32_t V = f.facts().num_vocab;
    if (kind.penalized) {
        wrk::penalize_rows(q, logits, V, V, B, f.penalty.par, f.penalty.out, V);
        logits = f.penalty.out;
    }
    // DRY: in place on the penalised row, else on a copy of the biased row or of head_o
    if (kind.dry) {
        float* rows = kind.penalized ? f.penalty.out : f.dry.out;
        if (!kind.penalized) wrk::copy_rows(q, logits, V, V, B, rows, V);
        wrk::dry_rows(q, rows, V, V, B, f.dry.par, f.dry.brk, f.dry.scratch);
        logits = rows;
    }
    // the mask: in place on the penalised or the DRY row, else from the biased row or head_o into grammar.out
    if (kind.constrained) {
        if (!f.grammar.holds({B, V}) || argmax_done) return wrk_fail(f.ctx, WRK_E_ARG, "grammar states are not prepared");
        float* masked = kind.penalized ? f.penalty.out : kind.dry ? f.dry.out : f.grammar.out;
        wrk::constrain_rows(q, logits, V, V, B, f.grammar.par, masked, V);
        logits = masked;
    }
    return WRK_OK;
}

// tail of a beam program's step, on the row the pick would be made on: the candidate front and beam_select, the permutation of the
// slots by the step's copy list, then the snapshot of the slots that ended in the step (their state after the permutation)
static int32_t enqueue_beam_tail(wrk_frame_common& f, uint32_t B, wrk_step_kind kind, const wrk_v7_state* st, uint32_t b0, const float* logits,
                                 bool argmax_done) {
    hipStream_t q = f.ctx->op_stream();
    const wrk::FrameIo& io = f.io();
    const uint32_t V = f.facts().num_vocab;
    const size_t slot = state_slot_floats(st);
    if (!f.beam.holds({B}) || f.beam.dim[3] != (size_t)st->num_layer * slot || b0 + B > st->num_batch || argmax_done)
        return wrk_fail(f.ctx, WRK_E_ARG, "beam buffers are not prepared");
    if (kind.sampled() || kind.logprobs || kind.stop_seqs || kind.guided)
        return wrk_fail(f.ctx, WRK_E_ARG, "a beam step composes with a logit bias and a context only");
    // a context: every slot's row goes through the stages of a pick's chain with the slot's own context
    const bool context = kind.penalized || kind.dry || kind.constrained;
    if (context && !f.beam_ctx.holds({B, kind.penalized ? (size_t)V : 0u}))
        return wrk_fail(f.ctx, WRK_E_ARG, "beam context rows are not prepared");
    if (kind.penalized && !f.penalty.holds({B, V})) return wrk_fail(f.ctx, WRK_E_ARG, "penalty rows are not prepared");
    const int32_t src = enqueue_context_rows(f, B, kind, logits, argmax_done);
    if (src != WRK_OK) return src;
    if (wrk::beam_step_rows(q, logits, V, V, B, io.tokens, f.beam.lp_par, f.beam.part, f.beam.keys, f.beam.dev(), io.tokens, io.counter, f.ctx->num_cu) != 0)
        return wrk_fail(f.ctx, WRK_E_UNSUPPORTED, "beam search: vocabulary of %u tokens", V);
    wrk::beam_permute(q, beam_state(st, b0), f.beam.scratch, st->num_layer, slot, f.beam.copy_src, B, f.ctx->num_cu);
    if (context) {
        // the contexts follow the hypotheses by the same copy list, and only then count the tokens the step gave out: io.tokens of the
        // slots it filled
        const wrk::BeamCtxRows rows{kind.penalized ? f.penalty.par : nullptr, kind.dry ? f.dry.par : nullptr, kind.constrained ? f.grammar.state : nullptr};
        wrk::beam_context_permute(q, rows, f.beam_ctx.dev(), V, f.beam.copy_src, B);
        const wrk::RowGate gate{f.beam.filled, 1u, 1u};
        if (kind.penalized) wrk::occurrence_update(q, V, B, f.penalty.par, io.tokens, 1, gate);
        if (kind.constrained) wrk::grammar_advance(q, V, B, f.grammar.par, io.tokens, gate);
        if (kind.dry) wrk::window_push(q, V, B, f.dry.par, io.tokens, gate);
    }
    wrk::beam_copy(q, beam_state(st, b0), wrk::BeamSlots{f.beam.snap, B, 0u}, st->num_layer, slot, f.beam.snap_map, false, B, f.ctx->num_cu);
    return WRK_OK;
}

int32_t wrk_enqueue_pick(wrk_frame_common& f, uint32_t frame_b, wrk_step_kind kind, const wrk_v7_state* st, uint32_t b0, bool argmax_done) {
    // the rows of the pick: a guided step ran 2B sequences, B conditional ones and their partners
    const uint32_t B = kind.guided ? frame_b / 2 : frame_b;
    hipStream_t q = f.ctx->op_stream();
    const wrk::FrameIo& io = f.io();
    const uint32_t V = f.facts().num_vocab;
    const float* logits = io.head_o;
    if (kind.dry && (!f.dry.holds({B, V}) || argmax_done)) return wrk_fail(f.ctx, WRK_E_ARG, "DRY rows are not prepared");
    // guidance in front of the bias: the guided rows of head_o's pairs (r, B + r) are what the rest reads; log-probs, last_logits and the
    // stop snapshot keep head_o
    if (kind.guided) {
        if (!f.guide.holds({B, V}) || argmax_done || frame_b != 2 * B || b0 != 0 || kind.pool() || kind.tail == wrk_step_kind::BEAM)
            return wrk_fail(f.ctx, WRK_E_ARG, "guidance rows are not prepared");
        wrk::guide_rows(q, io.head_o, V, V, B, f.guide.par, f.guide.out, V);
        logits = f.guide.out;
    }
    // the bias first: the biased copy of head_o (which log-probs, last_logits and the stop snapshot keep raw) is what the rest reads
    if (kind.biased) {
        if (!f.bias.holds({B, V}) || argmax_done) return wrk_fail(f.ctx, WRK_E_ARG, "bias rows are not prepared");
        wrk::bias_rows(q, logits, V, V, B, f.bias.par, f.bias.out, V);
        logits = f.bias.out;
    }
    if (kind.tail == wrk_step_kind::BEAM) return enqueue_beam_tail(f, B, kind, st, b0, logits, argmax_done);
    const int32_t src = enqueue_context_rows(f, B, kind, logits, argmax_done);
    if (src != WRK_OK) return src;
    // the sampler only reads the counter: rows run in different workgroups, so the tail's advance moves it after all of them
    if (!kind.sampled()) {
        if (!argmax_done) wrk::argmax_rows(q, logits, V, V, B, io.argmax);
    } else if (kind.filtered() && !f.filter.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "filter rows are not prepared");
    else if (kind.alt() && !f.alt.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "Mirostat / typical rows are not prepared");
    else if (kind.cut() && !f.cut_par.holds({B})) return wrk_fail(f.ctx, WRK_E_ARG, "cut rows are not prepared");
    else {
        // mu moves exactly where an occurrence row counts a draw: both read the step's one gate
        wrk::SamplePick pick{wrk::SAMPLE_PLAIN, f.sample.par, nullptr, nullptr, wrk::RowGate{nullptr, 0u, 0u}};
        if (kind.filtered()) { pick.mode = wrk::SAMPLE_FILT; pick.filt = f.filter.par; }
        if (kind.cut()) { pick.mode = wrk::SAMPLE_CUT; pick.cut = f.cut_par.par; }
        if (kind.alt()) { pick.mode = kind.mirostat() ? wrk::SAMPLE_MIRO : wrk::SAMPLE_TYP; pick.alt = f.alt.par; }
        if (kind.mirostat()) {
            const int32_t grc = draw_gate(f, B, kind, pick.gate);
            if (grc != WRK_OK) return grc;
        }
        const int rc = wrk::sample_rows(q, logits, V, V, B, pick, io.counter, io.argmax);
        if (rc != 0) return wrk_fail(f.ctx, WRK_E_UNSUPPORTED, "sampler: vocabulary of %u tokens", V);
    }
    // the picked tokens are in io.argmax and the tail has not moved the counter: row *counter of the frame's buffers, on the raw head output
    if (kind.logprobs) {
        if (!f.logprob.holds({0, B})) return wrk_fail(f.ctx, WRK_E_ARG, "log-prob buffers are not prepared");
        if (wrk::logprob_rows(q, io.head_o, V, V, B, io.argmax, io.counter, f.logprob.par, f.logprob.part, f.logprob.keys, f.ctx->num_cu) != 0)
            return wrk_fail(f.ctx, WRK_E_UNSUPPORTED, "log-probs: vocabulary of %u tokens", V);
    }
    if (kind.queue()) return enqueue_queue_tail(f, B, kind, st, b0);
    if (kind.tail == wrk_step_kind::STOP) return enqueue_stop_tail(f, frame_b, B, kind, st, b0);
    const int32_t urc = enqueue_draw_updates(f, B, kind);
    if (urc != WRK_OK) return urc;
    enqueue_guide_follow(f, B, kind);
    wrk::advance_tokens(q, io.argmax, io.tokens, f.history.tokens, io.counter, frame_b);
    return WRK_OK;
}

// ------------------------------------------------------------------ decode loops: lanes and the timed replay
// a pipeline of the timed replay: sequences [b0, b0 + nb) on their own frame; prog: its step program, or nullptr to enqueue eagerly
struct wrk_lane { wrk_frame_common* frame; uint32_t b0, nb; wrk_program* prog; };
// of a stop or queue call (kind.tail != PLAIN): what the polled loop cannot derive from the lanes and the kind
struct wrk_stop_run { uint32_t poll_steps; uint32_t* out_lengths; uint32_t* steps_run; };
static constexpr uint32_t WRK_STOP_POLL_DEFAULT = 16;

// Part 1 of a decode loop on lane `ln`: the frame, the upload of tokens / cursors / pick rows of its sequences, the buffers of the tail
// (stop: the call's stop rows, queue: its tables -- whichever kind.tail names) and, unless WRK_NO_GRAPH=1, the cached step program.
// Every group is grown before the look-up: growing a held group drops the programs.  One program per (state, first sequence, B, the runner's
// key bits, step kind -- key() in the mode word, key2() in the second): the analogue of the reference's cached RnnJob for a repeated RnnInfo
static int32_t lane_prepare(wrk_lane& ln, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t steps, uint32_t mode, wrk_step_kind kind,
                            const wrk_pick_params& rows, const wrk::StopParam* stop, const wrk_stopseq_pack* seq, const wrk_queue_pack* queue,
                            uint32_t num_top, const wrk_beam_pack* beam = nullptr) {
    wrk_frame_common& f = *ln.frame;
    const uint32_t b0 = ln.b0, B = ln.nb;
    int32_t rc = f.ensure_frame(B, mode);
    if (rc == WRK_OK) rc = wrk_decode_prepare(f, first_tokens, b0, B, steps, rows);
    if (rc == WRK_OK && kind.tail == wrk_step_kind::STOP) rc = wrk_stop_prepare(f, st, b0, B, stop + b0, seq);
    if (rc == WRK_OK && kind.queue()) rc = wrk_queue_prepare(f, st, B, *queue);
    if (rc == WRK_OK && kind.tail == wrk_step_kind::BEAM) rc = wrk_beam_prepare(f, st, B, *beam);
    if (rc == WRK_OK && kind.logprobs) rc = wrk_logprob_prepare(f, kind.guided ? B / 2 : B, steps, num_top);     // the rows of the pick
    ln.prog = nullptr;
    if (rc != WRK_OK || wrk_no_graph()) return rc;
    const wrk_frame_common::GraphKey key{st->uid, B | (b0 << 16), f.key_bits(B, mode) | kind.key(), 0u, kind.key2()};
    return wrk_cached_program(f.ctx, f.graphs, key, [&] { return f.enqueue_step(st, b0, B, mode, kind); }, &ln.prog);
}

// `steps` steps of every lane between two events: one lane on the submission stream (enqueued step by step without a program), several
// on lane 0's lane_streams[g], joined through lane_events[g].  A stop or queue tail: the polled loop of wrk_generate's comment on the
// tail's live count, then stop_restore and the lengths (stop).  Then tokens [steps][B] and last logits [B][V] come back, and into `lp`
// (when on) the log-prob rows of the steps that ran
static int32_t wrk_run_lanes(wrk_ctx* ctx, const std::vector<wrk_lane>& lanes, wrk_v7_state* st, uint32_t B, uint32_t steps, uint32_t mode,
                             wrk_step_kind kind, uint32_t* out_tokens, float* last_logits, float* elapsed_ms, const wrk_stop_run& stop,
                             const wrk_logprob_call& lp) {
    const size_t groups = lanes.size();
    const bool polled = kind.tail != wrk_step_kind::PLAIN;
    const std::vector<hipStream_t>& streams = lanes[0].frame->lane_streams;
    const std::vector<hipEvent_t>& events = lanes[0].frame->lane_events;
    const uint32_t V = lanes[0].frame->facts().num_vocab;
    // what comes back: the sequences of the call, in a guided one (one lane of 2R sequences) the R conditional ones, columns [0, R)
    const uint32_t OB = kind.guided ? B / 2 : B;
    auto out_rows = [&](const wrk_lane& ln) { return kind.guided ? ln.nb / 2 : ln.nb; };
    // every early return below leaves through this guard: the timing events are destroyed and, after an error, the lane streams are
    // drained (a lane's queued step programs must not outlive a frame that the next call may reallocate)
    struct Guard {
        wrk_ctx* ctx; const std::vector<hipStream_t>& streams; hipEvent_t e0 = nullptr, e1 = nullptr; bool ok = false;
        ~Guard() {
            if (!ok) { for (hipStream_t ls : streams) hipStreamSynchronize(ls); hipStreamSynchronize(ctx->stream); }
            if (e0) hipEventDestroy(e0);
            if (e1) hipEventDestroy(e1);
        }
    } guard{ctx, streams};
    WRK_HIP(ctx, hipEventCreate(&guard.e0));
    WRK_HIP(ctx, hipEventCreate(&guard.e1));
    hipEvent_t e0 = guard.e0, e1 = guard.e1;
    auto step = [&]() -> int32_t {      // one step of every lane
        if (groups == 1 && !lanes[0].prog) return lanes[0].frame->enqueue_step(st, 0, B, mode, kind);
        for (size_t g = 0; g < groups; ++g) WRK_HIP(ctx, hipGraphLaunch(lanes[g].prog->exec, groups == 1 ? ctx->stream : streams[g]));
        return WRK_OK;
    };
    uint32_t* live_host = nullptr;
    hipEvent_t* poll_events = nullptr;
    const bool beam = kind.tail == wrk_step_kind::BEAM;
    // the tail's live count: requests not yet ended / LIVE slots / sequences still running
    auto live_of = [&](const wrk_lane& ln) { return kind.queue() ? ln.frame->queue.live() : beam ? ln.frame->beam.live : ln.frame->stop.live(); };
    if (polled) {
        for (const wrk_lane& ln : lanes)
            if (!(kind.queue() ? ln.frame->queue.held() : beam ? ln.frame->beam.held() : ln.frame->stop.held()))
                return wrk_fail(ctx, WRK_E_ARG, "stop run on a lane without stop buffers");
        const int32_t rc = lanes[0].frame->ensure_poll((uint32_t)groups);
        if (rc != WRK_OK) return rc;
        live_host = lanes[0].frame->live_host;
        poll_events = lanes[0].frame->poll_events.data();
    }
    WRK_HIP(ctx, hipEventRecord(e0, ctx->stream));
    // several lanes: every lane replays its own step program on its own stream; the lanes start together behind e0 and the submission
    // stream joins them all before e1
    if (groups > 1)
        for (size_t g = 0; g < groups; ++g) WRK_HIP(ctx, hipStreamWaitEvent(streams[g], e0, 0));
    if (polled) {
        const uint32_t poll = stop.poll_steps ? stop.poll_steps : WRK_STOP_POLL_DEFAULT;
        uint32_t run = 0;
        for (uint32_t k = 0; run < steps; ++k) {
            if (k >= 2) {       // block k - 2 has been followed by a whole block of queued work: the wait is an event wait, short or none
                uint32_t live = 0;
                for (size_t g = 0; g < groups; ++g) {
                    WRK_HIP(ctx, hipEventSynchronize(poll_events[(k & 1) * groups + g]));
                    live += live_host[(k & 1) * groups + g];
                }
                if (live == 0) break;
            }
            const uint32_t n = steps - run < poll ? steps - run : poll;
            for (uint32_t i = 0; i < n; ++i) {
                const int32_t rc = step();
                if (rc != WRK_OK) return rc;
            }
            run += n;
            for (size_t g = 0; g < groups; ++g) {
                hipStream_t ls = groups == 1 ? ctx->stream : streams[g];
                WRK_HIP(ctx, hipMemcpyAsync(live_host + (k & 1) * groups + g, live_of(lanes[g]), 4, hipMemcpyDeviceToHost, ls));
                WRK_HIP(ctx, hipEventRecord(poll_events[(k & 1) * groups + g], ls));
            }
        }
        steps = run;
    } else {
        for (uint32_t i = 0; i < steps; ++i) {
            const int32_t rc = step();
            if (rc != WRK_OK) return rc;
        }
    }
    if (groups > 1)
        for (size_t g = 0; g < groups; ++g) {
            WRK_HIP(ctx, hipEventRecord(events[g], streams[g]));
            WRK_HIP(ctx, hipStreamWaitEvent(ctx->stream, events[g], 0));
        }
    WRK_HIP(ctx, hipEventRecord(e1, ctx->stream));
    WRK_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0.0f;
    WRK_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    if (elapsed_ms) *elapsed_ms = ms;
    if (kind.tail == wrk_step_kind::STOP) {
        // the frozen slots and logits rows go back (head_o is what the read-back below takes), the lengths come out
        for (const wrk_lane& ln : lanes) {
            wrk::stop_restore(ctx->stream, stop_geom(*ln.frame, st, ln.b0), ln.nb, ctx->num_cu);
            WRK_HIP(ctx, hipMemcpyAsync(stop.out_lengths + ln.b0, ln.frame->stop.lengths(), (size_t)out_rows(ln) * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        WRK_LAUNCH_CHECK(ctx);
    }
    if (beam) {
        // the frozen slots go back: every DONE slot's snapshot, taken by the step that ended it
        for (const wrk_lane& ln : lanes)
            wrk::beam_copy(ctx->stream, wrk::BeamSlots{ln.frame->beam.snap, ln.nb, 0u}, beam_state(st, ln.b0), st->num_layer, state_slot_floats(st),
                           ln.frame->beam.done_map, false, ln.nb, ctx->num_cu);
        WRK_LAUNCH_CHECK(ctx);
    }
    if (polled) *stop.steps_run = steps;
    for (const wrk_lane& ln : lanes) {
        const size_t onb = out_rows(ln);
        if (out_tokens) {
            if (groups == 1 && !kind.guided) WRK_HIP(ctx, hipMemcpyAsync(out_tokens, ln.frame->history.tokens, (size_t)steps * B * 4, hipMemcpyDeviceToHost, ctx->stream));
            else WRK_HIP(ctx, hipMemcpy2DAsync(out_tokens + ln.b0, (size_t)OB * 4, ln.frame->history.tokens, (size_t)ln.nb * 4, onb * 4, steps,
                                               hipMemcpyDeviceToHost, ctx->stream));
        }
        if (lp.on() && steps) {
            // rows [steps][nb] of the lane into [steps][B] at its first sequence; the top arrays the same with num_top entries per sequence
            const size_t n = lp.num_top;
            WRK_HIP(ctx, hipMemcpy2DAsync(lp.logprob + ln.b0, (size_t)OB * 4, ln.frame->logprob.logprob, onb * 4, onb * 4, steps,
                                          hipMemcpyDeviceToHost, ctx->stream));
            if (n) {
                WRK_HIP(ctx, hipMemcpy2DAsync(lp.top_ids + ln.b0 * n, OB * n * 4, ln.frame->logprob.top_ids, onb * n * 4, onb * n * 4, steps,
                                              hipMemcpyDeviceToHost, ctx->stream));
                WRK_HIP(ctx, hipMemcpy2DAsync(lp.top_logprobs + ln.b0 * n, OB * n * 4, ln.frame->logprob.top_logprobs, onb * n * 4, onb * n * 4, steps,
                                              hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        if (last_logits) WRK_HIP(ctx, hipMemcpyAsync(last_logits + (size_t)ln.b0 * V, ln.frame->io().head_o, onb * V * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    guard.ok = true;
    return WRK_OK;
}

// ------------------------------------------------------------------ decode loops: the two calls
int32_t wrk_generate(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t B, uint32_t steps,
                     const wrk_pick_args& pick, uint32_t* out_tokens, float* last_logits, float* elapsed_ms, uint32_t mode_arg,
                     const wrk_stop_call* stop) {
    if (!ctx) return WRK_E_ARG;
    LOCK(ctx);
    if (stop) {
        WRK_ARG(ctx, stop->opt, "options required");
        WRK_ARG(ctx, stop->out_lengths && stop->steps_run, "out_lengths and steps_run are required");
    }
    if (!m || !st || !first_tokens) return WRK_E_ARG;
    const uint32_t V = m->facts().num_vocab;
    wrk_step_kind kind;
    kind.tail = stop ? wrk_step_kind::STOP : wrk_step_kind::PLAIN;
    wrk_pick_params rows;
    std::vector<wrk::StopParam> stop_rows;      // generate_stop: one row per sequence
    wrk_logprob_call lp;
    if (stop) lp = wrk_logprob_call{stop->opt->num_top, stop->opt->out_logprob, stop->opt->out_top_ids, stop->opt->out_top_logprobs};
    int32_t rc = wrk_pick_pack(ctx, pick, B, B, V, rows, kind);
    if (rc == WRK_OK) rc = wrk_logprob_check(ctx, lp, V, kind);
    if (rc == WRK_OK && stop) rc = wrk_stop_sets(ctx, stop->opt->stop_tokens, stop->opt->stop_offsets, B, V, "sequence", stop_rows);
    wrk_stopseq_pack seq;                       // generate_stop with stop sequences: their rows and the tails the sequences start with
    if (rc == WRK_OK && stop) {
        const wrk_generate_options& o = *stop->opt;
        rc = wrk_stop_seqs(ctx, o.stop_seq_tokens, o.stop_seq_offsets, o.stop_seq_owners, o.out_stop_match || o.stop_tail, o.stop_tail, B, V, "sequence", seq);
        kind.stop_seqs = seq.on;
    }
    // Guidance: the frame runs FB = 2B sequences, the conditional ones on slots [0, B) and their partners, which the caller
    // fed the negative prompt, on slots [B, 2B).  Partner B + b gets the first token, the stop set, the stop-sequence row and the tail of
    // b, sees the same draws and so ends in the same step; the pick rows stay B
    const float* gscale = stop ? stop->opt->guidance_scale : nullptr;
    const uint32_t* gfirst = stop ? stop->opt->guidance_first_tokens : nullptr;
    std::vector<uint32_t> guided_first;
    uint32_t FB = B;
    if (rc == WRK_OK) WRK_ARG(ctx, gscale || !gfirst, "guidance_first_tokens without guidance_scale");
    if (rc == WRK_OK && gscale) {
        rc = wrk_guide_pack(ctx, gscale, B, V, rows.guide);
        if (rc != WRK_OK) return rc;
        WRK_ARG(ctx, B >= 1, "a guided call of no sequences");
        if (((mode_arg >> 8) & 0xffu) > 1) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "guidance on several lanes: a sequence and its partner share one frame");
        WRK_ARG(ctx, (uint64_t)2 * B <= st->num_batch, "guidance of %u sequences needs %u state slots, the state has %u", B, 2 * B, st->num_batch);
        kind.guided = true;
        FB = 2 * B;
        guided_first.assign(first_tokens, first_tokens + B);
        guided_first.insert(guided_first.end(), gfirst ? gfirst : first_tokens, (gfirst ? gfirst : first_tokens) + B);
        first_tokens = guided_first.data();
        // the partners' rows: rows [0, B) once more, through a copy (a range insert may not read from the vector it grows)
        auto twice = [](auto& v) { const auto head = v; v.insert(v.end(), head.begin(), head.end()); };
        twice(stop_rows);
        if (seq.on) { twice(seq.rows); twice(seq.tails); }
    }
    if (rc == WRK_OK) rc = wrk_generate_check(ctx, st, m->facts(), first_tokens, FB);
    if (rc != WRK_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0f;
    if (stop) {
        *stop->steps_run = 0;
        for (uint32_t b = 0; b < B; ++b) stop->out_lengths[b] = 0;
        for (uint32_t b = 0; b < B && stop->opt->out_stop_match; ++b) stop->opt->out_stop_match[b] = WRK_STOP_MATCH_NONE;
    }
    if (steps == 0) return WRK_OK;
    // mode: bits 0-7 = 0 op-by-op / 1 fused; bits 8-15 = number of concurrent pipelines the sequences are dealt over (0, 1: one)
    const uint32_t mode = mode_arg & 0xffu;
    uint32_t groups = (mode_arg >> 8) & 0xffu;
    if (groups > m->max_lanes()) groups = m->max_lanes();
    if (groups < 1) groups = 1;
    if (groups > B) groups = B;
    if (kind.guided) groups = 1;
    WRK_ARG(ctx, groups == 1 || !wrk_no_graph(), "concurrent pipelines replay captured programs: not with WRK_NO_GRAPH=1");
    m->before_loop();
    std::vector<wrk_lane> L(groups);
    for (uint32_t g = 0; g < groups; ++g) {
        rc = m->lane(g, groups, &L[g].frame);
        if (rc != WRK_OK) return rc;
        L[g].b0 = (uint32_t)((uint64_t)FB * g / groups);
        L[g].nb = (uint32_t)((uint64_t)FB * (g + 1) / groups) - L[g].b0;
        // lane g uploads the parameters of its own sequences: a sequence's tokens do not depend on the number of lanes
        rc = lane_prepare(L[g], st, first_tokens, steps, mode, kind, rows, stop_rows.data(), seq.on ? &seq : nullptr, nullptr, lp.num_top);
        if (rc != WRK_OK) return rc;
    }
    const wrk_stop_run run{stop ? stop->opt->poll_steps : 0u, stop ? stop->out_lengths : nullptr, stop ? stop->steps_run : nullptr};
    rc = wrk_run_lanes(ctx, L, st, FB, steps, mode, kind, out_tokens, last_logits, elapsed_ms, run, lp);
    if (rc != WRK_OK) return rc;
    // rows of a lane that come back: its sequences, in a guided call (one lane of 2B) the B conditional ones, the lane's leading half
    auto back_rows = [&](const wrk_lane& ln) { return kind.guided ? B : ln.nb; };
    if (kind.mirostat() && pick.mirostat_mu) {      // every lane's rows hold the mu after the draws that counted
        for (const wrk_lane& ln : L) {
            WRK_HIP(ctx, hipMemcpy(rows.alt.data() + ln.b0, ln.frame->alt.par, (size_t)back_rows(ln) * sizeof(wrk::SampleAlt), hipMemcpyDeviceToHost));
            for (uint32_t b = ln.b0; b < ln.b0 + back_rows(ln); ++b) pick.mirostat_mu[b] = rows.alt[b].mu;
        }
    }
    if (kind.constrained && pick.grammar_state)     // every lane's words hold the states after the draws that counted
        for (const wrk_lane& ln : L)
            WRK_HIP(ctx, hipMemcpy(pick.grammar_state + ln.b0, ln.frame->grammar.state, (size_t)back_rows(ln) * 4, hipMemcpyDeviceToHost));
    if (kind.stop_seqs)                             // and the match words and the tails, frozen with the sequences that ended
        for (const wrk_lane& ln : L) {
            if (stop->opt->out_stop_match)
                WRK_HIP(ctx, hipMemcpy(stop->opt->out_stop_match + ln.b0, ln.frame->stop_seq.match, (size_t)back_rows(ln) * 4, hipMemcpyDeviceToHost));
            if (stop->opt->stop_tail)
                WRK_HIP(ctx, hipMemcpy(stop->opt->stop_tail + (size_t)ln.b0 * WRK_STOP_TAIL_LEN, ln.frame->stop_seq.tail,
                                       (size_t)back_rows(ln) * WRK_STOP_TAIL_LEN * 4, hipMemcpyDeviceToHost));
        }
    return m->after_loop(groups);
}

int32_t wrk_generate_queue(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                           const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, wrk_step_kind::Tail tail,
                           const wrk_queue_pool* pool, const wrk_queue_guidance* guide, bool guided, const wrk_queue_cuts* cuts) {
    if (!ctx || !m || !st) return WRK_E_ARG;
    LOCK(ctx);
    wrk_queue_result out = out_arg ? *out_arg : wrk_queue_result{};
    wrk_queue_pack pk;
    int32_t rc = wrk_queue_check(ctx, opt, st, B, m->facts().num_vocab, mode_arg, out_arg ? &out : nullptr, pk, guided, cuts);
    if (rc == WRK_OK && tail != wrk_step_kind::QUEUE_POOL && opt->history) rc = wrk_fail(ctx, WRK_E_ARG, "a history pool without a state pool");
    if (rc == WRK_OK && tail == wrk_step_kind::QUEUE_POOL) rc = wrk_queue_pool_check(ctx, pool, opt, st, m->facts().num_vocab, pk);
    if (rc == WRK_OK && guided) rc = wrk_queue_guide_check(ctx, guide, opt, st, m->facts().num_vocab, pk);
    if (rc != WRK_OK) return rc;
    wrk_queue_start(opt, B, pk);
    const uint32_t FB = pk.kind.guided ? 2 * B : B;         // the sequences of the frame: a guided queue runs B pairs
    rc = wrk_generate_check(ctx, st, m->facts(), pk.first_tokens.data(), FB);
    if (rc != WRK_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0f;
    const uint32_t mode = mode_arg & 0xffu;
    m->before_loop();
    std::vector<wrk_lane> L{{nullptr, 0, FB, nullptr}};     // one lane: a queue shared by several streams would need cross-stream atomics
    rc = m->lane(0, 1, &L[0].frame);
    if (rc == WRK_OK) rc = lane_prepare(L[0], st, pk.first_tokens.data(), pk.max_steps, mode, pk.kind, pk.rows, nullptr, nullptr, &pk, pk.lp.num_top);
    if (rc != WRK_OK) return rc;
    uint32_t steps_run = 0;
    rc = wrk_run_lanes(ctx, L, st, FB, pk.max_steps, mode, pk.kind, nullptr, nullptr, elapsed_ms, wrk_stop_run{pk.poll_steps, nullptr, &steps_run}, wrk_logprob_call{});
    if (rc == WRK_OK) rc = m->after_loop(1);
    if (rc != WRK_OK) return rc;
    return wrk_queue_finish(*m, B, steps_run, pk, opt, &out);
}

int32_t wrk_generate_queue_cut(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, uint32_t B, const wrk_queue_options* opt,
                               const wrk_queue_result* out_arg, float* elapsed_ms, uint32_t mode_arg, const wrk_queue_cuts* cuts) {
    if (!ctx || !m || !st) return WRK_E_ARG;
    {
        LOCK(ctx);
        WRK_ARG(ctx, cuts, "cuts required");
        WRK_ARG(ctx, !cuts->pool || !cuts->guide, "a state pool under a guided queue: no entry point takes both");
    }
    const wrk_step_kind::Tail tail = cuts->pool ? wrk_step_kind::QUEUE_POOL : wrk_step_kind::QUEUE;
    return wrk_generate_queue(ctx, m, st, B, opt, out_arg, elapsed_ms, mode_arg, tail, cuts->pool, cuts->guide, cuts->guide != nullptr, cuts);
}

// the context of wrk_v*_generate_beam_context validated into pk.rows: one value per group becomes one row per slot, slot q
// of the call naming slot q of the table and of the window.  Sets kind.penalized / dry / constrained; an empty context sets nothing
static int32_t wrk_beam_context_check(wrk_ctx* ctx, const wrk_beam_context& c, uint32_t G, uint32_t W, uint32_t V, wrk_beam_pack& pk, wrk_step_kind& kind) {
    const uint32_t B = G * W;
    WRK_ARG(ctx, c.occ || (!c.presence && !c.frequency && !c.decay), "penalty arrays without an occurrence table");
    WRK_ARG(ctx, c.grammar || (!c.grammar_state && !c.out_grammar_state), "grammar_state / out_grammar_state without grammar");
    wrk_dry_args dry{c.window, c.dry_multiplier, c.dry_base, c.dry_allowed_length, c.no_repeat_ngram, c.dry_breakers, c.num_dry_breakers};
    WRK_ARG(ctx, c.window || !dry.any_array(), "dry_* / no_repeat_ngram arrays without a token window");
    // a group's value for each of its slots
    auto per_slot = [&](auto* group, auto& slots) {
        slots.clear();
        for (uint32_t q = 0; group && q < B; ++q) slots.push_back(group[q / W]);
        return group ? slots.data() : nullptr;
    };
    if (c.occ) {
        std::vector<float> pres, freq, dec;
        WRK_ARG(ctx, c.occ->num_batch >= B, "occurrence table of %u slots, %u beam slots", c.occ->num_batch, B);
        const int32_t rc = wrk_penalty_pack(ctx, c.occ, 0, B, V, per_slot(c.presence, pres), per_slot(c.frequency, freq), per_slot(c.decay, dec), pk.rows.pen);
        if (rc != WRK_OK) return rc;
        kind.penalized = true;
        pk.ctx_vocab = V;
    }
    if (c.window) {
        std::vector<float> mult, base;
        std::vector<uint32_t> allowed, nr;
        WRK_ARG(ctx, c.window->num_batch >= B, "token window of %u slots, %u beam slots", c.window->num_batch, B);
        dry.multiplier = per_slot(c.dry_multiplier, mult); dry.base = per_slot(c.dry_base, base);
        dry.allowed_length = per_slot(c.dry_allowed_length, allowed); dry.no_repeat_ngram = per_slot(c.no_repeat_ngram, nr);
        const int32_t rc = wrk_dry_pack(ctx, dry, 0, B, B, V, pk.rows.dry, pk.rows.brk);
        if (rc != WRK_OK) return rc;
        kind.dry = pk.rows.has_dry = true;
        pk.ctx_capacity = c.window->capacity;
    }
    if (c.grammar) {
        std::vector<uint32_t> start;
        const int32_t rc = wrk_grammar_pack(ctx, c.grammar, per_slot(c.grammar_state, start), B, V, pk.rows.gram_state);
        if (rc != WRK_OK) return rc;
        kind.constrained = true;
        pk.rows.grammar = c.grammar;
        pk.out_grammar_state = c.out_grammar_state;
    }
    return WRK_OK;
}

// generate_beam: opt validated into pk (WRK_E_ARG / WRK_E_UNSUPPORTED before any launch); sets kind
static int32_t wrk_beam_check(wrk_ctx* ctx, const wrk_beam_options* opt, const wrk_beam_result* out, const wrk_v7_state* st, const uint32_t* first_tokens,
                              uint32_t G, uint32_t steps, uint32_t V, uint32_t mode_arg, const wrk_beam_context* bc, wrk_beam_pack& pk,
                              wrk_step_kind& kind) {
    WRK_ARG(ctx, opt, "options required");
    WRK_ARG(ctx, out && out->tokens && out->lengths && out->scores && out->finished && out->slots && out->num_hyps && out->steps_run,
            "every result array but the step arrays is required");
    const uint32_t W = opt->num_beams;
    WRK_ARG(ctx, W >= 1 && W <= WRK_MAX_BEAMS, "num_beams %u: must be in [1, %u]", W, (uint32_t)WRK_MAX_BEAMS);
    WRK_ARG(ctx, G >= 1 && (uint64_t)G * W <= st->num_batch && (uint64_t)G * W <= 256, "%u groups of %u beams: at most min(%u, 256) slots", G, W,
            st->num_batch);
    WRK_ARG(ctx, steps >= 1, "steps 0");
    WRK_ARG(ctx, ((mode_arg >> 8) & 0xffu) <= 1, "generate_beam runs on one lane");
    static const wrk_generate_options none{};
    const wrk_generate_options& g = opt->gen ? *opt->gen : none;
    WRK_ARG(ctx, !g.temperature && !g.top_p && !g.seed && !g.top_k && !g.min_p && !g.mirostat_tau && !g.mirostat_eta && !g.mirostat_mu && !g.typical_p &&
                     !wrk_cut_of(g).any(),
            "beam search takes no sampler");
    WRK_ARG(ctx, !g.presence && !g.frequency && !g.decay && !g.occ, "beam search takes penalties in a wrk_beam_context, not in gen");
    WRK_ARG(ctx, !g.window && !g.dry_multiplier && !g.dry_base && !g.dry_allowed_length && !g.no_repeat_ngram && !g.dry_breakers && !g.num_dry_breakers,
            "beam search takes DRY / the n-gram ban in a wrk_beam_context, not in gen");
    WRK_ARG(ctx, !g.grammar && !g.grammar_state, "beam search takes a grammar in a wrk_beam_context, not in gen");
    WRK_ARG(ctx, !g.num_top && !g.out_logprob && !g.out_top_ids && !g.out_top_logprobs, "beam search returns no log-prob rows");
    WRK_ARG(ctx, !g.stop_seq_tokens && !g.stop_seq_offsets && !g.stop_seq_owners && !g.out_stop_match && !g.stop_tail, "beam search takes no stop sequences");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "beam search: vocabulary of %u tokens", V);
    if (g.guidance_scale || g.guidance_first_tokens)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "beam search with guidance: the permutation would have to move the partner slots too");
    const uint32_t B = G * W;
    pk.G = G; pk.W = W; pk.steps = steps; pk.poll_steps = g.poll_steps;
    int32_t rc = wrk_beam_inv_norm(ctx, opt->length_penalty, steps, pk.inv_norm);
    if (rc == WRK_OK) rc = wrk_beam_stops(ctx, g.stop_tokens, g.stop_offsets, G, V, pk.stops);
    wrk_pick_params per_group;
    wrk_pick_args pick;
    pick.bias = g.bias; pick.bias_set = g.bias_set;
    kind = wrk_step_kind{};
    if (rc == WRK_OK) rc = wrk_pick_pack(ctx, pick, G, G, V, per_group, kind);
    if (rc != WRK_OK) return rc;
    kind.tail = wrk_step_kind::BEAM;
    pk.rows.bias = per_group.bias;
    pk.first_tokens.resize(B);
    pk.slots.assign(B, wrk::BeamSlot{-INFINITY, -INFINITY, 0u, (uint32_t)WRK_BEAM_DEAD});
    for (uint32_t q = 0; q < B; ++q) {
        pk.first_tokens[q] = first_tokens[q / W];
        if (kind.biased) pk.rows.bias_set.push_back(per_group.bias_set[q / W]);
        if (q % W == 0) pk.slots[q] = wrk::BeamSlot{0.0f, 0.0f, 0u, (uint32_t)WRK_BEAM_LIVE};
    }
    return bc ? wrk_beam_context_check(ctx, *bc, G, W, V, pk, kind) : WRK_OK;
}

// after the loop and the restore: the records and the history rows come back; per group the non-DEAD slots by key descending, ties by
// slot, each backtracked through the parents
static int32_t wrk_beam_finish(wrk_frame_common& f, const wrk_beam_pack& pk, uint32_t steps_run, const wrk_beam_result& out) {
    wrk_ctx* ctx = f.ctx;
    const uint32_t G = pk.G, W = pk.W, B = G * W;
    const size_t rows = (size_t)steps_run * B;
    std::vector<wrk::BeamSlot> slots(B);
    std::vector<uint32_t> tok(rows), par(rows);
    WRK_HIP(ctx, hipMemcpyAsync(slots.data(), f.beam.slots, (size_t)B * sizeof(wrk::BeamSlot), hipMemcpyDeviceToHost, ctx->stream));
    if (rows) {
        WRK_HIP(ctx, hipMemcpyAsync(tok.data(), f.beam.step_tokens, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        WRK_HIP(ctx, hipMemcpyAsync(par.data(), f.beam.step_parents, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        if (out.step_scores) WRK_HIP(ctx, hipMemcpyAsync(out.step_scores, f.beam.step_scores, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (pk.out_grammar_state) WRK_HIP(ctx, hipMemcpyAsync(pk.out_grammar_state, f.grammar.state, (size_t)B * 4, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out.step_tokens && rows) memcpy(out.step_tokens, tok.data(), rows * 4);
    if (out.step_parents && rows) memcpy(out.step_parents, par.data(), rows * 4);
    for (uint32_t g = 0; g < G; ++g) {
        std::vector<uint32_t> order;
        for (uint32_t q = g * W; q < (g + 1) * W; ++q)
            if (slots[q].status != WRK_BEAM_DEAD) order.push_back(q);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return slots[a].key > slots[b].key; });
        out.num_hyps[g] = (uint32_t)order.size();
        for (uint32_t r = 0; r < W; ++r) {
            const size_t at = (size_t)g * W + r;
            uint32_t* dst = out.tokens + at * pk.steps;
            for (uint32_t j = 0; j < pk.steps; ++j) dst[j] = 0u;
            out.lengths[at] = 0u; out.scores[at] = 0.0f; out.finished[at] = 0u; out.slots[at] = WRK_BEAM_NO_TOKEN;
            if (r >= order.size()) continue;
            const uint32_t q = order[r];
            const wrk::BeamSlot& s = slots[q];
            uint32_t cur = q, left = s.length;
            // nothing below can leave the rows that ran or the group unless the device history is wrong
            for (uint32_t t = steps_run; t-- > 0 && left > 0;) {
                const uint32_t y = tok[(size_t)t * B + cur], p = par[(size_t)t * B + cur];
                if (p / W != g) return wrk_fail(ctx, WRK_E_HIP, "slot %u: inconsistent beam history at step %u (parent %u)", q, t, p);
                if (y != WRK_BEAM_NO_TOKEN) dst[--left] = y;
                cur = p;
            }
            if (left != 0 || s.length > pk.steps) return wrk_fail(ctx, WRK_E_HIP, "slot %u: inconsistent beam history (length %u)", q, s.length);
            out.lengths[at] = s.length; out.scores[at] = s.score; out.finished[at] = s.status == WRK_BEAM_DONE; out.slots[at] = q;
        }
    }
    *out.steps_run = steps_run;
    return WRK_OK;
}

int32_t wrk_generate_beam(wrk_ctx* ctx, wrk_frame_common* m, wrk_v7_state* st, const uint32_t* first_tokens, uint32_t G, uint32_t steps,
                          const wrk_beam_options* opt, const wrk_beam_result* out_arg, float* elapsed_ms, uint32_t mode_arg,
                          const wrk_beam_context* bc) {
    if (!ctx || !m || !st || !first_tokens) return WRK_E_ARG;
    LOCK(ctx);
    const uint32_t V = m->facts().num_vocab;
    wrk_beam_pack pk;
    wrk_step_kind kind;
    int32_t rc = wrk_beam_check(ctx, opt, out_arg, st, first_tokens, G, steps, V, mode_arg, bc, pk, kind);
    const uint32_t B = pk.G * pk.W;
    if (rc == WRK_OK) rc = wrk_generate_check(ctx, st, m->facts(), pk.first_tokens.data(), B);
    if (rc != WRK_OK) return rc;
    if (elapsed_ms) *elapsed_ms = 0.0f;
    const uint32_t mode = mode_arg & 0xffu;
    m->before_loop();
    std::vector<wrk_lane> L{{nullptr, 0, B, nullptr}};
    rc = m->lane(0, 1, &L[0].frame);
    if (rc == WRK_OK) rc = lane_prepare(L[0], st, pk.first_tokens.data(), steps, mode, kind, pk.rows, nullptr, nullptr, nullptr, 0u, &pk);
    if (rc != WRK_OK) return rc;
    uint32_t steps_run = 0;
    rc = wrk_run_lanes(ctx, L, st, B, steps, mode, kind, nullptr, nullptr, elapsed_ms, wrk_stop_run{pk.poll_steps, nullptr, &steps_run}, wrk_logprob_call{});
    if (rc == WRK_OK) rc = m->after_loop(1);
    if (rc != WRK_OK) return rc;
    return wrk_beam_finish(*L[0].frame, pk, steps_run, *out_arg);
}
