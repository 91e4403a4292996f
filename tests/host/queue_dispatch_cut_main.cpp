// Host driver of the cut words of the request queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch): reads
// cases from stdin, runs one dispatch per case over host arrays pre-filled with a canary, and prints the slots' cut rows and every other
// word the arrays then hold as one JSON line.  Built and run by tests/test_queue_dispatch_cut_host.py, which holds the expectations.
//
// A case is one line:
//   case name B R r b first_step cut
// cut: 1 hands in the slots' SampleCut rows, 0 hands in nullptr.  Request i has the prompt of i + 1 tokens 100 + 10 i .., max_new 4 + i,
// seed 1000 + i, temperature 0.5 + 0.25 i, top_p 0.5, top_k 3 + i, ln_min_p -1 - i and the five cut words 1 + i, -2 - i, -3 - i,
// 0.125 (1 + i), -4 - i (top_n_sigma, ln_epsilon, ln_eta, xtc_probability, ln_xtc_threshold).  The call has a sampler and a filter and
// none of the other features.  Every word a dispatch may write starts as CANARY.
#include "wrk_queue_dispatch.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace wrk;

template <class T> static void fill(std::vector<T>& v) { memset(v.data(), 0xA5, v.size() * sizeof(T)); }

template <class T> static std::string words(const std::vector<T>& v) {      // every 32-bit word of v
    static_assert(sizeof(T) % 4 == 0, "words");
    std::vector<uint32_t> w(v.size() * sizeof(T) / 4);
    if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 4);
    std::string s = "[";
    for (size_t i = 0; i < w.size(); ++i) s += (i ? "," : "") + std::to_string(w[i]);
    return s + "]";
}

int main() {
    static_assert(sizeof(SampleCut) == 20, "five words");
    std::string line, tag, name;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream cs(line);
        uint32_t B, R, r, b, first_step, cut;
        cs >> tag >> name >> B >> R >> r >> b >> first_step >> cut;
        if (tag != "case" || !cs) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        std::vector<QueueReq> reqs(R);
        std::vector<uint32_t> ids;
        for (uint32_t i = 0; i < R; ++i) {
            QueueReq& q = reqs[i];
            memset(&q, 0, sizeof q);
            const float f = (float)i;
            q.prompt_off = (uint32_t)ids.size(); q.prompt_len = i + 1; q.max_new = 4 + i; q.seed = 1000 + i;
            q.temperature = 0.5f + 0.25f * f; q.top_p = 0.5f;
            q.top_k = 3 + i; q.ln_min_p = -1.0f - f;
            q.top_n_sigma = 1.0f + f; q.ln_epsilon = -2.0f - f; q.ln_eta = -3.0f - f; q.xtc_probability = 0.125f * (1.0f + f);
            q.ln_xtc_threshold = -4.0f - f;
            for (uint32_t k = 0; k <= i; ++k) ids.push_back(100 + 10 * i + k);
        }
        std::vector<uint32_t> tokens(B);
        std::vector<QueueSlot> slots(B);
        std::vector<QueueLog> log(R);
        std::vector<SampleParam> par(B);
        std::vector<SampleFilter> filt(B);
        std::vector<SampleCut> cuts(B);
        fill(tokens); fill(slots); fill(log); fill(par); fill(filt); fill(cuts);
        const std::vector<QueueReq> reqs_in = reqs;
        QueueBufs Q{};
        Q.slots = slots.data(); Q.reqs = reqs.data(); Q.pool = ids.data(); Q.log = log.data();
        Q.sample_par = par.data(); Q.filter_par = filt.data();
        if (cut) Q.cut_par = cuts.data();
        const bool wipe = queue_dispatch(Q, tokens.data(), r, b, first_step, nullptr);
        const bool kept = memcmp(reqs.data(), reqs_in.data(), R * sizeof(QueueReq)) == 0;       // the requests are only read
        std::printf("{\"name\":\"%s\",\"wipe\":%s,\"requests_kept\":%s,\"cut\":%s,\"filter\":%s,\"tokens\":%s,\"slots\":%s,\"log\":%s,\"sample\":%s}\n",
                    name.c_str(), wipe ? "true" : "false", kept ? "true" : "false", words(cuts).c_str(), words(filt).c_str(),
                    words(tokens).c_str(), words(slots).c_str(), words(log).c_str(), words(par).c_str());
    }
    return 0;
}
