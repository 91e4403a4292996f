// Host driver of the bias word of the request queue's dispatch rule (web-rwkv-gguf_amd/csrc/wrk_queue_dispatch.h queue_dispatch): reads
// cases from stdin, runs one dispatch per case over host arrays pre-filled with a canary, and prints the bias words and every other word
// the arrays then hold as one JSON line.  Built and run by tests/test_queue_dispatch_bias_host.py, which holds the expectations.
//
// A case is one line:
//   case name B R r b first_step bias w_0 .. w_{R-1}
// bias: 1 hands in the slots' and the requests' bias words, 0 hands in nullptr for both; w_i: request i's bias set word.  Request i has
// the prompt of i + 1 tokens 100 + 10 i .., max_new 4 + i, seed 1000 + i, temperature 0.5 + 0.25 i, top_p 0.5, automaton state 7 + i.  The
// call has a sampler and a grammar and none of the other features.  Every word a dispatch may write starts as CANARY.
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
    std::string line, tag, name;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::stringstream cs(line);
        uint32_t B, R, r, b, first_step, bias;
        cs >> tag >> name >> B >> R >> r >> b >> first_step >> bias;
        std::vector<uint32_t> bias_req(R);
        for (uint32_t i = 0; i < R; ++i) cs >> bias_req[i];
        if (tag != "case" || !cs) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        std::vector<QueueReq> reqs(R);
        std::vector<uint32_t> gram(R), ids;
        for (uint32_t i = 0; i < R; ++i) {
            QueueReq& q = reqs[i];
            memset(&q, 0, sizeof q);
            q.prompt_off = (uint32_t)ids.size(); q.prompt_len = i + 1; q.max_new = 4 + i; q.seed = 1000 + i;
            q.temperature = 0.5f + 0.25f * (float)i; q.top_p = 0.5f;
            for (uint32_t k = 0; k <= i; ++k) ids.push_back(100 + 10 * i + k);
            gram[i] = 7 + i;
        }
        std::vector<uint32_t> tokens(B), gram_state(B), bias_set(B);
        std::vector<QueueSlot> slots(B);
        std::vector<QueueLog> log(R);
        std::vector<SampleParam> par(B);
        fill(tokens); fill(gram_state); fill(bias_set); fill(slots); fill(log); fill(par);
        const std::vector<uint32_t> bias_in = bias_req, gram_in = gram;
        QueueBufs Q{};
        Q.slots = slots.data(); Q.reqs = reqs.data(); Q.pool = ids.data(); Q.log = log.data();
        Q.sample_par = par.data();
        Q.gram_state = gram_state.data(); Q.gram_req = gram.data();
        if (bias) { Q.bias_set = bias_set.data(); Q.bias_req = bias_req.data(); }
        const bool wipe = queue_dispatch(Q, tokens.data(), r, b, first_step, nullptr);
        const bool kept = bias_req == bias_in && gram == gram_in;       // the requests' own entries are only read
        std::printf("{\"name\":\"%s\",\"wipe\":%s,\"requests_kept\":%s,\"bias_set\":%s,\"tokens\":%s,\"slots\":%s,\"log\":%s,\"sample\":%s,"
                    "\"gram_state\":%s}\n",
                    name.c_str(), wipe ? "true" : "false", kept ? "true" : "false", words(bias_set).c_str(), words(tokens).c_str(),
                    words(slots).c_str(), words(log).c_str(), words(par).c_str(), words(gram_state).c_str());
    }
    return 0;
}
