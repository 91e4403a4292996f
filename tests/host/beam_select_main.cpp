// Host driver of beam search's pure rule (web-rwkv-gguf_amd/csrc/wrk_beam_select.h beam_select_group): reads groups from stdin, runs one
// step per group over output arrays of exactly W entries pre-filled with a canary, and prints everything they then hold as one JSON line.
// Built and run by tests/test_beam_select_host.py, which holds the expectations (tests/beam_ref.py).
//
// A group is a `case` line, an `inv` line, a `stop` line, W `slot` lines and W `row` lines; every float travels as its bits:
//   case name W
//   inv  n bits ...                          the inv_norm table, entries [0, n)
//   stop n id ...                            ascending
//   slot score_bits key_bits length status
//   row  id lp_bits  id lp_bits ...          W pairs: the slot's W first tokens and their log-probs
#include "wrk_beam_select.h"

#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace wrk;

static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

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
        uint32_t W = 0;
        cs >> tag >> name >> W;
        if (tag != "case" || !cs || W < 1 || W > WRK_MAX_BEAMS) { std::fprintf(stderr, "bad case line: %s\n", line.c_str()); return 2; }
        std::getline(std::cin, line);
        std::stringstream is(line);
        size_t n = 0;
        is >> tag >> n;
        std::vector<float> inv(n);
        for (size_t i = 0; i < n; ++i) { uint32_t u = 0; is >> u; inv[i] = from_bits(u); }
        if (tag != "inv" || !is) { std::fprintf(stderr, "bad inv line: %s\n", line.c_str()); return 2; }
        std::getline(std::cin, line);
        std::stringstream ss(line);
        BeamStop stop{};
        ss >> tag >> stop.count;
        if (tag != "stop" || !ss || stop.count > WRK_MAX_BEAM_STOP_TOKENS) { std::fprintf(stderr, "bad stop line: %s\n", line.c_str()); return 2; }
        for (uint32_t i = 0; i < stop.count; ++i) ss >> stop.ids[i];
        std::vector<BeamSlot> in(W);
        for (uint32_t b = 0; b < W; ++b) {
            std::getline(std::cin, line);
            std::stringstream rs(line);
            uint32_t sb = 0, kb = 0;
            rs >> tag >> sb >> kb >> in[b].length >> in[b].status;
            if (tag != "slot" || !rs) { std::fprintf(stderr, "bad slot line: %s\n", line.c_str()); return 2; }
            in[b].score = from_bits(sb); in[b].key = from_bits(kb);
        }
        std::vector<uint32_t> ids((size_t)W * W);
        std::vector<float> lp((size_t)W * W);
        for (uint32_t b = 0; b < W; ++b) {
            std::getline(std::cin, line);
            std::stringstream rs(line);
            rs >> tag;
            for (uint32_t j = 0; j < W; ++j) { uint32_t u = 0; rs >> ids[b * W + j] >> u; lp[b * W + j] = from_bits(u); }
            if (tag != "row" || !rs) { std::fprintf(stderr, "bad row line: %s\n", line.c_str()); return 2; }
        }
        const std::vector<BeamSlot> in_before = in;
        std::vector<BeamSlot> out(W);
        std::vector<uint32_t> token(W), parent(W), ended(W);
        fill(out); fill(token); fill(parent); fill(ended);
        beam_select_group(in.data(), W, ids.data(), lp.data(), inv.data(), stop, out.data(), token.data(), parent.data(), ended.data());
        const bool kept = memcmp(in.data(), in_before.data(), W * sizeof(BeamSlot)) == 0;      // the records handed in are only read
        std::printf("{\"name\":\"%s\",\"inputs_kept\":%s,\"slots\":%s,\"token\":%s,\"parent\":%s,\"ended\":%s}\n", name.c_str(), kept ? "true" : "false",
                    words(out).c_str(), words(token).c_str(), words(parent).c_str(), words(ended).c_str());
    }
    return 0;
}
