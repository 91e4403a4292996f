// Stand-alone driver of web-rwkv-gguf_amd/csrc/wrk_regex.h for tests/test_regex_host.py: the header alone, no HIP, built under the address
// and undefined-behaviour sanitizers.  Commands on stdin, one JSON object per command on stdout:
//   compile N DUMP          then N lines, a pattern each in hex ("-": the empty pattern)
//       -> {"rc", "err", "num_states", "starts", "accepting", "next" (rows of 256, only with DUMP = 1)}
//   arrays S P              then S * 256 next entries, S accepting flags, P starts -> {"rc", "num_states", "byte_classes"}
//   tokens S P V END WEAK   then the arrays as above and V lines, a token each in hex: the host half of wrk_grammar_compile (byte classes,
//                           grouping, verify, token-level trim) around a plain walk -> {"rc", "lost", "num_states", "num_classes",
//                           "byte_classes", "rounds", "final", "token_class", "starts", "transitions"}
//   group V MAX            then V hashes (decimal u64) and V column ids: the true column of every token, which the verify callback
//                           compares as the device's third pass compares walks -> {"rc", "classes", "reps", "rounds", "verify_calls"}
#include <inttypes.h>
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "wrk_regex.h"

static std::string unhex(const std::string& h) {
    std::string out;
    if (h == "-") return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return out;
}

static uint64_t mix(uint64_t x) {          // SplitMix64's finalizer: a sum of these over a column's entries does not depend on the order
    x *= 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static std::string json_escape(const std::string& s) {
    std::string out;
    for (unsigned char c : s) {
        if (c == '"' || c == '\\') { out.push_back('\\'); out.push_back((char)c); }
        else if (c < 0x20 || c >= 0x7F) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); out += b; }
        else out.push_back((char)c);
    }
    return out;
}

template <class T>
static void put_list(const char* name, const T* v, size_t n, bool comma = true) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < n; ++i) printf("%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    printf("]%s", comma ? ", " : "");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "compile") {
            uint32_t n = 0, dump = 0;
            in >> n >> dump;
            std::vector<std::string> pats(n);
            for (uint32_t i = 0; i < n; ++i) { std::getline(std::cin, line); pats[i] = unhex(line); }
            std::vector<const char*> ptr(n);
            std::vector<size_t> len(n);
            for (uint32_t i = 0; i < n; ++i) { ptr[i] = pats[i].data(); len[i] = pats[i].size(); }
            wrk_byte_dfa d;
            std::string msg;
            const int32_t rc = wrk::regex_compile(ptr.data(), len.data(), n, d, msg);
            printf("{\"rc\": %d, \"err\": \"%s\", \"num_states\": %u, ", rc, json_escape(msg).c_str(), d.num_states);
            put_list("starts", d.starts.data(), d.starts.size());
            put_list("accepting", d.accepting.data(), d.accepting.size());
            printf("\"next\": [");
            for (uint32_t s = 0; dump && s < d.num_states; ++s) {
                printf("%s[", s ? ", " : "");
                for (uint32_t b = 0; b < 256; ++b) printf("%s%u", b ? "," : "", (unsigned)d.next[(size_t)s * 256 + b]);
                printf("]");
            }
            printf("]}\n");
        } else if (cmd == "arrays") {
            uint32_t S = 0, P = 0;
            in >> S >> P;
            std::vector<uint16_t> next((size_t)S * 256);
            std::vector<uint8_t> acc(S);
            std::vector<uint32_t> starts(P);
            for (auto& v : next) { unsigned x; std::cin >> x; v = (uint16_t)x; }
            for (auto& v : acc) { unsigned x; std::cin >> x; v = (uint8_t)x; }
            for (auto& v : starts) std::cin >> v;
            std::getline(std::cin, line);
            wrk_byte_dfa d;
            const int32_t rc = wrk::byte_dfa_from_arrays(S, next.data(), acc.data(), starts.data(), P, d);
            uint32_t bc = 0;
            if (rc == WRK_OK) {
                uint8_t cls[256];
                std::vector<uint16_t> table;
                bc = wrk::byte_dfa_compress(d, cls, table);
            }
            printf("{\"rc\": %d, \"num_states\": %u, \"byte_classes\": %u}\n", rc, d.num_states, bc);
        } else if (cmd == "tokens") {
            // the host half of wrk_grammar_compile around a plain walk on this thread: byte classes, grouping by a column hash
            // (WEAK = 1: the number of allowed states, so different columns collide), verify, token-level trim
            uint32_t S = 0, P = 0, V = 0, end = 0, weak = 0;
            in >> S >> P >> V >> end >> weak;
            std::vector<uint16_t> next((size_t)S * 256);
            std::vector<uint8_t> acc(S);
            std::vector<uint32_t> starts(P);
            for (auto& v : next) { unsigned x; std::cin >> x; v = (uint16_t)x; }
            for (auto& v : acc) { unsigned x; std::cin >> x; v = (uint8_t)x; }
            for (auto& v : starts) std::cin >> v;
            std::getline(std::cin, line);
            std::vector<std::string> vocab(V);
            for (uint32_t t = 0; t < V; ++t) { std::getline(std::cin, line); vocab[t] = unhex(line); }
            wrk_byte_dfa d;
            int32_t rc = wrk::byte_dfa_from_arrays(S, next.data(), acc.data(), starts.data(), P, d);
            uint8_t cls[256];
            std::vector<uint16_t> table;
            const uint32_t BC = rc == WRK_OK ? wrk::byte_dfa_compress(d, cls, table) : 0;
            auto column = [&](uint32_t t) {
                std::vector<uint16_t> col(S + 1, (uint16_t)WRK_GRAMMAR_REJECT);
                for (uint32_t s = 0; s <= S; ++s) {
                    uint32_t cur = s;
                    if (s == S) cur = t == end ? S : WRK_GRAMMAR_REJECT;
                    else if (t == end) cur = acc[s] ? S : WRK_GRAMMAR_REJECT;
                    else if (vocab[t].empty()) cur = WRK_GRAMMAR_REJECT;
                    else for (unsigned char b : vocab[t]) { cur = table[(size_t)cur * BC + cls[b]]; if (cur == WRK_GRAMMAR_REJECT) break; }
                    col[s] = (uint16_t)cur;
                }
                return col;
            };
            std::vector<std::vector<uint16_t>> cols(V);
            std::vector<uint64_t> hash(V, 0);
            for (uint32_t t = 0; rc == WRK_OK && t < V; ++t) {
                cols[t] = column(t);
                for (uint32_t s = 0; s <= S; ++s)
                    if (cols[t][s] != WRK_GRAMMAR_REJECT) hash[t] += weak ? 1 : mix(((uint64_t)s << 16 | cols[t][s]) + 1);
            }
            uint32_t rounds = 0;
            auto verify = [&](const std::vector<uint32_t>& tc, const std::vector<uint32_t>& reps, std::vector<uint32_t>& bad) -> int32_t {
                for (uint32_t t = 0; t < V; ++t) if (cols[t] != cols[reps[tc[t]]]) bad.push_back(t);
                return WRK_OK;
            };
            std::vector<uint32_t> tc, reps, keep;
            std::vector<uint16_t> trans;
            uint32_t NS = 0, NC = 0;
            if (rc == WRK_OK) rc = wrk::group_token_classes(hash.data(), V, WRK_MAX_TOKEN_CLASSES, tc, reps, verify, &rounds);
            int lost = -1;
            if (rc == WRK_OK) {
                const uint32_t C = (uint32_t)reps.size();
                std::vector<uint16_t> walk((size_t)(S + 1) * C);
                for (uint32_t c = 0; c < C; ++c) for (uint32_t s = 0; s <= S; ++s) walk[(size_t)s * C + c] = cols[reps[c]][s];
                wrk::token_trim(S, C, walk, tc, trans, NS, NC, keep);
                for (uint32_t p = 0; p < P; ++p) { if (keep[starts[p]] == UINT32_MAX && lost < 0) lost = (int)p; starts[p] = keep[starts[p]]; }
            }
            printf("{\"rc\": %d, \"lost\": %d, \"num_states\": %u, \"num_classes\": %u, \"byte_classes\": %u, \"rounds\": %u, \"final\": %u, ", rc, lost, NS, NC, BC,
                   rounds, keep.empty() ? 0u : keep[S]);
            put_list("token_class", tc.data(), tc.size());
            put_list("starts", starts.data(), starts.size());
            put_list("transitions", trans.data(), trans.size(), false);
            printf("}\n");
        } else if (cmd == "group") {
            uint32_t V = 0, max_classes = 0;
            in >> V >> max_classes;
            std::vector<uint64_t> hash(V);
            std::vector<uint32_t> col(V);
            for (auto& v : hash) std::cin >> v;
            for (auto& v : col) std::cin >> v;
            std::getline(std::cin, line);
            uint32_t calls = 0, rounds = 0;
            auto verify = [&](const std::vector<uint32_t>& tc, const std::vector<uint32_t>& reps, std::vector<uint32_t>& bad) -> int32_t {
                ++calls;
                for (uint32_t t = 0; t < V; ++t)
                    if (col[t] != col[reps[tc[t]]]) bad.push_back(t);
                return WRK_OK;
            };
            std::vector<uint32_t> tc, reps;
            const int32_t rc = wrk::group_token_classes(hash.data(), V, max_classes, tc, reps, verify, &rounds);
            printf("{\"rc\": %d, ", rc);
            put_list("classes", tc.data(), tc.size());
            put_list("reps", reps.data(), reps.size());
            printf("\"rounds\": %u, \"verify_calls\": %u}\n", rounds, calls);
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}
