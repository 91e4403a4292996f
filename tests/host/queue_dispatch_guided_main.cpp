// Host driver of the guided queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch_guided): reads cases from
// stdin, runs one dispatch per case over host arrays pre-filled with a canary, and prints everything the arrays then hold as one JSON
// line.  Built and run by tests/test_queue_dispatch_guided_host.py, which holds the expectations.
//
// A case is a `case` line, R `req` lines and a `pool` line:
//   case name rule B R r b first_step off
//   req  prompt_off prompt_len max_new seed temperature top_p presence frequency decay top_k ln_min_p tau eta typical_p
//        mu gram from dry_allowed dry_no_repeat dry_multiplier dry_pen0 neg_off neg_len scale
//   pool n id ...
// rule: `guided` runs queue_dispatch_guided for pair b of B (every per-slot array of the rule 2B long, every per-pair array B), `plain`
// runs queue_dispatch for slot b over the same arrays with a QueueBufs that names none of the guided arrays: what the rule wrote before
// they existed.  off: a comma list of the optional arrays handed in as nullptr -- sample, pen, filter, alt, mu, gram, dry, seq, intake --
// or `-`.  A request's DRY table is pen[m] = dry_pen0 + m.  Every word a dispatch may write starts as CANARY, every pointer of a slot's
// row as a canary address that is never dereferenced; floats are printed as their bits.
#include "wrk_queue_dispatch.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace wrk;

static const uintptr_t PTR_CANARY = (uintptr_t)0x5A5A5A50u;

template <class T> static void fill(std::vector<T>& v) { memset(v.data(), 0xA5, v.size() * sizeof(T)); }
static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

template <class T> static std::string words(const std::vector<T>& v) {      // every 32-bit word of v
    static_assert(sizeof(T) % 4 == 0, "words");
    std::vector<uint32_t> w(v.size() * sizeof(T) / 4);
    if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 4);
    std::string s = "[";
    for (size_t i = 0; i < w.size(); ++i) s += (i ? "," : "") + std::to_string(w[i]);
    return s + "]";
}

int main() {
    std::string line, tag, name, rule, off;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream cs(line);
        uint32_t B, R, r, b, first_step;
        cs >> tag >> name >> rule >> B >> R >> r >> b >> first_step >> off;
        if (tag != "case" || !cs || (rule != "guided" && rule != "plain")) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        std::vector<QueueReq> reqs(R);
        std::vector<float> mu(R), scale_req(R);
        std::vector<uint32_t> gram(R), from(R), neg_off(R), neg_len(R), ids;
        std::vector<DryParam> dry_req(R);
        for (uint32_t i = 0; i < R; ++i) {
            std::getline(std::cin, line);
            std::stringstream rs(line);
            QueueReq& q = reqs[i];
            DryParam& d = dry_req[i];
            memset(&q, 0, sizeof q);
            memset(&d, 0, sizeof d);
            float pen0 = 0.0f;
            rs >> tag >> q.prompt_off >> q.prompt_len >> q.max_new >> q.seed >> q.temperature >> q.top_p >> q.presence >> q.frequency >> q.decay >>
                q.top_k >> q.ln_min_p >> q.tau >> q.eta >> q.typical_p >> mu[i] >> gram[i] >> from[i] >> d.allowed >> d.no_repeat >> d.multiplier >>
                pen0 >> neg_off[i] >> neg_len[i] >> scale_req[i];
            if (tag != "req" || !rs) { std::fprintf(stderr, "bad req line: %s\n", line.c_str()); return 2; }
            for (uint32_t m = 0; m <= WRK_DRY_MAX_MATCH; ++m) d.pen[m] = pen0 + (float)m;
            d.pen[WRK_DRY_MAX_MATCH + 1] = 777.0f;
        }
        std::getline(std::cin, line);
        std::stringstream ps(line);
        size_t n = 0;
        ps >> tag >> n;
        ids.resize(n);
        for (size_t i = 0; i < n; ++i) ps >> ids[i];
        if (tag != "pool" || !ps) { std::fprintf(stderr, "bad pool line: %s\n", line.c_str()); return 2; }

        const uint32_t S = 2 * B;       // slot records, tokens and start flags of a guided queue
        std::vector<uint32_t> tokens(S), started(S), pair_started(B), gram_state(B), tail((size_t)B * WRK_STOP_TAIL_LEN), take(B), seq_match(R);
        std::vector<float> scale(B);
        std::vector<QueueSlot> slots(S);
        std::vector<QueueLog> log(R);
        std::vector<SampleParam> par(B);
        std::vector<SampleFilter> filt(B);
        std::vector<SampleAlt> alt(B);
        std::vector<PenaltyParam> pen(B);
        std::vector<DryParam> dry(B);
        fill(tokens); fill(started); fill(pair_started); fill(gram_state); fill(tail); fill(take); fill(seq_match); fill(scale); fill(slots);
        fill(log); fill(par); fill(filt); fill(alt); fill(pen); fill(dry);
        for (uint32_t i = 0; i < B; ++i) {
            pen[i].count = (float*)PTR_CANARY; pen[i].flags = (uint8_t*)PTR_CANARY; pen[i].weight = (const float*)PTR_CANARY;
            dry[i].ring = (uint32_t*)PTR_CANARY; dry[i].meta = (uint32_t*)PTR_CANARY;
        }
        const std::vector<float> mu_in = mu, scale_in = scale_req;
        const std::vector<uint32_t> gram_in = gram, neg_off_in = neg_off, neg_len_in = neg_len;
        auto on = [&](const char* what) { return ("," + off + ",").find(std::string(",") + what + ",") == std::string::npos; };
        // the initializer of the rule's callers before the guided arrays existed: they keep their nullptr defaults
        QueueBufs Q{slots.data(), reqs.data(), ids.data(), log.data(), nullptr, started.data(),
                    on("sample") ? par.data() : nullptr, on("pen") ? pen.data() : nullptr, on("filter") ? filt.data() : nullptr,
                    on("alt") ? alt.data() : nullptr, on("mu") ? mu.data() : nullptr,
                    on("gram") ? gram_state.data() : nullptr, on("gram") ? gram.data() : nullptr,
                    on("dry") ? dry.data() : nullptr, on("dry") ? dry_req.data() : nullptr,
                    nullptr, on("seq") ? tail.data() : nullptr, on("seq") ? seq_match.data() : nullptr,
                    on("intake") ? from.data() : nullptr, on("intake") ? take.data() : nullptr};
        bool wipe = false;
        uint32_t start_cond = 0, start_part = 0;
        if (rule == "plain") {
            if (Q.neg_off || Q.neg_len || Q.scale_req || Q.scale || Q.pair_started) { std::fprintf(stderr, "guided arrays without being named\n"); return 2; }
            wipe = queue_dispatch(Q, tokens.data(), r, b, first_step, nullptr);
        } else {
            Q.neg_off = neg_off.data(); Q.neg_len = neg_len.data(); Q.scale_req = scale_req.data(); Q.scale = scale.data();
            Q.pair_started = pair_started.data();
            const QueuePairStart ps = queue_dispatch_guided(Q, tokens.data(), r, b, B, first_step);
            wipe = ps.wipe; start_cond = ps.start_cond; start_part = ps.start_part;
        }

        // the requests' own entries are only read
        bool kept = mu == mu_in && gram == gram_in && neg_off == neg_off_in && neg_len == neg_len_in && scale_req == scale_in;
        for (uint32_t i = 0; i < B; ++i) {
            kept = kept && pen[i].count == (float*)PTR_CANARY && pen[i].flags == (uint8_t*)PTR_CANARY && pen[i].weight == (const float*)PTR_CANARY;
            kept = kept && dry[i].ring == (uint32_t*)PTR_CANARY && dry[i].meta == (uint32_t*)PTR_CANARY;
        }
        std::vector<uint32_t> pen_vals, dry_vals;        // the rows without their pointers
        for (uint32_t i = 0; i < B; ++i) {
            pen_vals.insert(pen_vals.end(), {bits(pen[i].presence), bits(pen[i].frequency), bits(pen[i].decay), pen[i].pad});
            dry_vals.insert(dry_vals.end(), {dry[i].cap, dry[i].allowed, dry[i].no_repeat, bits(dry[i].multiplier)});
            for (float x : dry[i].pen) dry_vals.push_back(bits(x));
        }
        std::printf("{\"name\":\"%s\",\"wipe\":%s,\"start_cond\":%u,\"start_part\":%u,\"pointers_kept\":%s,\"tokens\":%s,\"started\":%s,"
                    "\"pair_started\":%s,\"scale\":%s,\"slots\":%s,\"log\":%s,\"sample\":%s,\"filter\":%s,\"alt\":%s,\"gram_state\":%s,\"tail\":%s,"
                    "\"take\":%s,\"seq_match\":%s,\"pen\":%s,\"dry\":%s}\n",
                    name.c_str(), wipe ? "true" : "false", start_cond, start_part, kept ? "true" : "false", words(tokens).c_str(),
                    words(started).c_str(), words(pair_started).c_str(), words(scale).c_str(), words(slots).c_str(), words(log).c_str(),
                    words(par).c_str(), words(filt).c_str(), words(alt).c_str(), words(gram_state).c_str(), words(tail).c_str(),
                    words(take).c_str(), words(seq_match).c_str(), words(pen_vals).c_str(), words(dry_vals).c_str());
    }
    return 0;
}
