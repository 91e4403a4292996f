// Regex -> byte DFA and the exact grouping of token columns (include/wrk_hip.h wrk_regex_compile / wrk_grammar_compile),
// free of HIP: a host test compiles this header alone.  wrk_grammar_compile.hip includes it.
//
// Pipeline per pattern: parse (a tree of byte sets, concatenation, alternation, repeats) -> Thompson NFA -> subset construction over
// the byte classes that the pattern's sets induce -> trim (states that reach no accepting state go, so a missing transition is
// REJECT and there is no dead state) -> Moore minimisation -> breadth-first renumbering from the start in byte order.  The alphabet is
// bytes, matching is whole-string.  A code point outside ASCII is its UTF-8 byte sequence; ".", a negated class and \D \W \S accept
// every well-formed UTF-8 sequence (no surrogates, no overlong forms, at most U+10FFFF) they do not exclude.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "wrk_hip.h"

// the byte DFA: next[s][byte] is a state or WRK_GRAMMAR_REJECT; pattern p owns the states [starts[p], starts[p + 1]) when it comes from
// wrk_regex_compile
struct wrk_byte_dfa {
    uint32_t num_states = 0;
    std::vector<uint16_t> next;         // [num_states][256]
    std::vector<uint8_t> accepting;     // [num_states]
    std::vector<uint32_t> starts;       // [num_patterns]
};

namespace wrk {

static constexpr uint32_t REGEX_MAX_STATES = 65534;         // byte-DFA states of one automaton: FINAL and REJECT keep their u16 values
static constexpr uint32_t REGEX_MAX_REPEAT = 1000;
static constexpr uint32_t REGEX_MAX_DEPTH = 200;            // nested groups
static constexpr uint32_t REGEX_MAX_NFA = 1u << 20;         // NFA states of one pattern

struct RegexError {
    int32_t code = WRK_OK;
    size_t offset = 0;
    std::string what;
    // "unsupported: look-around at offset 3" / "syntax: missing ) at offset 7"
    std::string text(uint32_t pattern) const {
        char buf[256];
        snprintf(buf, sizeof buf, "pattern %u: %s: %s at offset %zu", pattern, code == WRK_E_UNSUPPORTED ? "unsupported" : "syntax", what.c_str(),
                 offset);
        return buf;
    }
};

typedef std::array<uint64_t, 4> ByteSet;
inline void bs_add(ByteSet& s, uint32_t b) { s[b >> 6] |= 1ull << (b & 63); }
inline bool bs_has(const ByteSet& s, uint32_t b) { return (s[b >> 6] >> (b & 63)) & 1; }
inline ByteSet bs_range(uint32_t lo, uint32_t hi) {
    ByteSet s{};
    for (uint32_t b = lo; b <= hi; ++b) bs_add(s, b);
    return s;
}

// ----------------------------------------------------------------------------- the tree
struct RegexNode {
    enum Kind { EMPTY, SET, CAT, ALT, REPEAT } kind = EMPTY;
    ByteSet set{};
    std::vector<int> kids;
    uint32_t lo = 0, hi = 0;            // REPEAT: hi == UINT32_MAX is unbounded
};

// a set of code points: the ASCII members and whether every code point outside ASCII belongs to it
struct CodeSet { ByteSet ascii{}; bool rest = false; };

class RegexParser {
public:
    RegexParser(const uint8_t* p, size_t n) : p_(p), n_(n) {}
    std::vector<RegexNode> nodes;
    RegexError err;

    int parse() {           // the root, or -1 with err set
        const int root = alt(0);
        if (root >= 0 && i_ < n_) return fail(WRK_E_ARG, i_, "unmatched )");
        return root;
    }

private:
    const uint8_t* p_;
    size_t n_, i_ = 0;

    int fail(int32_t code, size_t off, const char* what) {
        if (err.code == WRK_OK) { err.code = code; err.offset = off; err.what = what; }
        return -1;
    }
    int add(RegexNode::Kind k) { nodes.emplace_back(); nodes.back().kind = k; return (int)nodes.size() - 1; }
    int set_node(const ByteSet& s) { const int n = add(RegexNode::SET); nodes[n].set = s; return n; }
    int cat2(int a, int b) { const int n = add(RegexNode::CAT); nodes[n].kids = {a, b}; return n; }
    int seq(const ByteSet& a, const ByteSet& b) { const int x = set_node(a); const int y = set_node(b); return cat2(x, y); }
    int seq(const ByteSet& a, const ByteSet& b, const ByteSet& c) { const int x = seq(a, b); const int y = set_node(c); return cat2(x, y); }
    int seq(const ByteSet& a, const ByteSet& b, const ByteSet& c, const ByteSet& d) { const int x = seq(a, b, c); const int y = set_node(d); return cat2(x, y); }

    // every well-formed UTF-8 sequence of two to four bytes
    int multibyte() {
        const ByteSet t = bs_range(0x80, 0xBF);
        const int n = add(RegexNode::ALT);
        std::vector<int> k;
        k.push_back(seq(bs_range(0xC2, 0xDF), t));
        k.push_back(seq(bs_range(0xE0, 0xE0), bs_range(0xA0, 0xBF), t));
        k.push_back(seq(bs_range(0xE1, 0xEC), t, t));
        k.push_back(seq(bs_range(0xED, 0xED), bs_range(0x80, 0x9F), t));
        k.push_back(seq(bs_range(0xEE, 0xEF), t, t));
        k.push_back(seq(bs_range(0xF0, 0xF0), bs_range(0x90, 0xBF), t, t));
        k.push_back(seq(bs_range(0xF1, 0xF3), t, t, t));
        k.push_back(seq(bs_range(0xF4, 0xF4), bs_range(0x80, 0x8F), t, t));
        nodes[n].kids = k;
        return n;
    }
    int code_set(const CodeSet& c) {
        const int a = set_node(c.ascii);
        if (!c.rest) return a;
        const int m = multibyte();
        const int n = add(RegexNode::ALT);
        nodes[n].kids = {a, m};
        return n;
    }

    static bool class_escape(uint8_t c, CodeSet& out) {
        CodeSet s;
        const uint8_t l = c | 0x20;
        if (l == 'd') s.ascii = bs_range('0', '9');
        else if (l == 'w') {
            s.ascii = bs_range('0', '9');
            for (uint32_t b = 'a'; b <= 'z'; ++b) { bs_add(s.ascii, b); bs_add(s.ascii, b - 32); }
            bs_add(s.ascii, '_');
        } else if (l == 's') {
            for (uint8_t b : {' ', '\t', '\n', '\r', '\f', '\v'}) bs_add(s.ascii, b);
        } else return false;
        if (c != l) negate(s);
        out = s;
        return true;
    }
    static void negate(CodeSet& s) {
        s.ascii[0] = ~s.ascii[0]; s.ascii[1] = ~s.ascii[1]; s.ascii[2] = s.ascii[3] = 0;
        s.rest = !s.rest;
    }
    static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : (c | 0x20) >= 'a' && (c | 0x20) <= 'f' ? (c | 0x20) - 'a' + 10 : -1; }

    // the escape at p_[i_] == '\\'.  1: one byte in `byte`; 2: a class in `cs`; -1: failed
    int escape(uint32_t& byte, CodeSet& cs) {
        const size_t at = i_;
        if (i_ + 1 >= n_) { fail(WRK_E_ARG, at, "\\ at the end"); return -1; }
        const uint8_t c = p_[i_ + 1];
        i_ += 2;
        switch (c) {
        case 'n': byte = '\n'; return 1;
        case 'r': byte = '\r'; return 1;
        case 't': byte = '\t'; return 1;
        case 'f': byte = '\f'; return 1;
        case 'v': byte = '\v'; return 1;
        case 'x': {
            if (i_ + 1 >= n_ || hex(p_[i_]) < 0 || hex(p_[i_ + 1]) < 0) { fail(WRK_E_ARG, at, "\\x needs two hex digits"); return -1; }
            byte = (uint32_t)(hex(p_[i_]) * 16 + hex(p_[i_ + 1]));
            i_ += 2;
            return 1;
        }
        case 'b': case 'B': case 'A': case 'Z': case 'z': fail(WRK_E_UNSUPPORTED, at, "anchor or word boundary"); return -1;
        case 'p': case 'P': fail(WRK_E_UNSUPPORTED, at, "Unicode property class"); return -1;
        default: break;
        }
        if (c >= '1' && c <= '9') { fail(WRK_E_UNSUPPORTED, at, "back-reference"); return -1; }
        if (class_escape(c, cs)) return 2;
        if (c >= 0x80 || c == '0' || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')) { fail(WRK_E_ARG, at, "unknown escape"); return -1; }
        byte = c;           // an escaped metacharacter or other ASCII punctuation
        return 1;
    }

    // one code point of the pattern text outside ASCII, as the concatenation of its bytes
    int utf8_literal() {
        const size_t at = i_;
        const uint8_t b0 = p_[i_];
        const uint32_t len = b0 >= 0xF0 ? 4 : b0 >= 0xE0 ? 3 : 2;
        bool ok = b0 >= 0xC2 && b0 <= 0xF4 && i_ + len <= n_;
        for (uint32_t k = 1; ok && k < len; ++k) ok = (p_[i_ + k] & 0xC0) == 0x80;
        if (ok) {
            const uint8_t b1 = p_[i_ + 1];
            ok = !(b0 == 0xE0 && b1 < 0xA0) && !(b0 == 0xED && b1 > 0x9F) && !(b0 == 0xF0 && b1 < 0x90) && !(b0 == 0xF4 && b1 > 0x8F);
        }
        if (!ok) return fail(WRK_E_ARG, at, "the pattern is not UTF-8");
        int n = set_node(bs_range(b0, b0));
        for (uint32_t k = 1; k < len; ++k) { const int t = set_node(bs_range(p_[i_ + k], p_[i_ + k])); n = cat2(n, t); }
        i_ += len;
        return n;
    }

    int char_class() {          // p_[i_] == '['
        const size_t open = i_++;
        CodeSet cs;
        bool neg = false;
        if (i_ < n_ && p_[i_] == '^') { neg = true; ++i_; }
        bool first = true;
        for (;; first = false) {
            if (i_ >= n_) return fail(WRK_E_ARG, open, "missing ]");
            if (p_[i_] == ']' && !first) { ++i_; break; }
            uint32_t lo = 0;
            CodeSet sub;
            const size_t at = i_;
            int kind = 1;
            if (p_[i_] == '\\') { kind = escape(lo, sub); if (kind < 0) return -1; }
            else lo = p_[i_++];
            if (kind == 2) {
                for (int w = 0; w < 2; ++w) cs.ascii[w] |= sub.ascii[w];
                cs.rest |= sub.rest;
                if (i_ + 1 < n_ && p_[i_] == '-' && p_[i_ + 1] != ']') return fail(WRK_E_ARG, at, "a class escape as a range end");
                continue;
            }
            if (lo >= 0x80) return fail(WRK_E_UNSUPPORTED, at, "non-ASCII class member");
            uint32_t hi = lo;
            if (i_ + 1 < n_ && p_[i_] == '-' && p_[i_ + 1] != ']') {
                ++i_;
                const size_t hat = i_;
                CodeSet dummy;
                if (p_[i_] == '\\') { const int k = escape(hi, dummy); if (k < 0) return -1; if (k == 2) return fail(WRK_E_ARG, hat, "a class escape as a range end"); }
                else hi = p_[i_++];
                if (hi >= 0x80) return fail(WRK_E_UNSUPPORTED, hat, "non-ASCII class member");
                if (hi < lo) return fail(WRK_E_ARG, at, "reversed range");
            }
            for (uint32_t b = lo; b <= hi; ++b) bs_add(cs.ascii, b);
        }
        if (neg) negate(cs);
        return code_set(cs);
    }

    int group(uint32_t depth) {         // p_[i_] == '('
        const size_t open = i_++;
        if (depth >= REGEX_MAX_DEPTH) return fail(WRK_E_UNSUPPORTED, open, "groups nested too deeply");
        if (i_ < n_ && p_[i_] == '?') {
            const uint8_t c = i_ + 1 < n_ ? p_[i_ + 1] : 0, d = i_ + 2 < n_ ? p_[i_ + 2] : 0;
            if (c == ':') i_ += 2;
            else if (c == '=' || c == '!' || (c == '<' && (d == '=' || d == '!'))) return fail(WRK_E_UNSUPPORTED, open, "look-around");
            else if (c == 'P' || c == '<' || c == '\'') return fail(WRK_E_UNSUPPORTED, open, "named group");
            else if (c == 0) return fail(WRK_E_ARG, open, "missing )");
            else return fail(WRK_E_UNSUPPORTED, open, "inline flags");
        }
        const int inner = alt(depth + 1);
        if (inner < 0) return -1;
        if (i_ >= n_ || p_[i_] != ')') return fail(WRK_E_ARG, open, "missing )");
        ++i_;
        return inner;
    }

    int atom(uint32_t depth) {
        const uint8_t c = p_[i_];
        const size_t at = i_;
        switch (c) {
        case '(': return group(depth);
        case '[': return char_class();
        case '.': {
            ++i_;
            CodeSet cs;
            bs_add(cs.ascii, '\n');
            negate(cs);
            return code_set(cs);
        }
        case '^': case '$': return fail(WRK_E_UNSUPPORTED, at, "anchor or word boundary");
        case '*': case '+': case '?': return fail(WRK_E_ARG, at, "nothing to repeat");
        case '{': return fail(WRK_E_ARG, at, "{ outside a quantifier (escape it)");
        case '\\': {
            uint32_t byte = 0;
            CodeSet cs;
            const int k = escape(byte, cs);
            if (k < 0) return -1;
            return k == 1 ? set_node(bs_range(byte, byte)) : code_set(cs);
        }
        default: break;
        }
        if (c >= 0x80) return utf8_literal();
        ++i_;
        return set_node(bs_range(c, c));
    }

    // the quantifiers that follow an atom
    int repeat(uint32_t depth) {
        int a = atom(depth);
        if (a < 0) return -1;
        bool had = false;
        while (i_ < n_) {
            const uint8_t c = p_[i_];
            const size_t at = i_;
            uint32_t lo, hi;
            if (c == '*') { lo = 0; hi = UINT32_MAX; ++i_; }
            else if (c == '+') { lo = 1; hi = UINT32_MAX; ++i_; }
            else if (c == '?') { lo = 0; hi = 1; ++i_; }
            else if (c == '{') {
                size_t j = i_ + 1;
                auto number = [&](uint32_t& v) {
                    const size_t b = j;
                    uint64_t x = 0;
                    while (j < n_ && p_[j] >= '0' && p_[j] <= '9' && j - b < 9) x = x * 10 + (p_[j++] - '0');
                    v = (uint32_t)x;
                    return j > b && !(j < n_ && p_[j] >= '0' && p_[j] <= '9');
                };
                if (!number(lo)) return fail(WRK_E_ARG, at, "malformed {m,n}");
                hi = lo;
                if (j < n_ && p_[j] == ',') {
                    ++j;
                    if (j < n_ && p_[j] == '}') hi = UINT32_MAX;
                    else if (!number(hi)) return fail(WRK_E_ARG, at, "malformed {m,n}");
                }
                if (j >= n_ || p_[j] != '}') return fail(WRK_E_ARG, at, "malformed {m,n}");
                if (hi != UINT32_MAX && hi < lo) return fail(WRK_E_ARG, at, "{m,n} with n < m");
                if (lo > REGEX_MAX_REPEAT || (hi != UINT32_MAX && hi > REGEX_MAX_REPEAT)) return fail(WRK_E_UNSUPPORTED, at, "repeat count above 1000");
                i_ = j + 1;
            } else break;
            if (had) return fail(WRK_E_ARG, at, "multiple repeat");
            if (i_ < n_ && (p_[i_] == '?' || p_[i_] == '+')) return fail(WRK_E_UNSUPPORTED, i_, "lazy or possessive quantifier");
            const int r = add(RegexNode::REPEAT);
            nodes[r].kids = {a};
            nodes[r].lo = lo; nodes[r].hi = hi;
            a = r;
            had = true;
        }
        return a;
    }

    int cat(uint32_t depth) {
        std::vector<int> k;
        while (i_ < n_ && p_[i_] != '|' && p_[i_] != ')') {
            const int r = repeat(depth);
            if (r < 0) return -1;
            k.push_back(r);
        }
        if (k.empty()) return add(RegexNode::EMPTY);
        if (k.size() == 1) return k[0];
        const int n = add(RegexNode::CAT);
        nodes[n].kids = k;
        return n;
    }

    int alt(uint32_t depth) {
        std::vector<int> k;
        for (;;) {
            const int c = cat(depth);
            if (c < 0) return -1;
            k.push_back(c);
            if (i_ < n_ && p_[i_] == '|') { ++i_; continue; }
            break;
        }
        if (k.size() == 1) return k[0];
        const int n = add(RegexNode::ALT);
        nodes[n].kids = k;
        return n;
    }
};

// ----------------------------------------------------------------------------- Thompson NFA
struct RegexNfa {
    struct State { std::vector<uint32_t> eps; int set = -1; uint32_t to = 0; };
    std::vector<State> st;
    std::vector<ByteSet> sets;
    bool overflow = false;

    uint32_t fresh() {
        if (st.size() >= REGEX_MAX_NFA) { overflow = true; return 0; }
        st.emplace_back();
        return (uint32_t)st.size() - 1;
    }
    // the fragment of node n entered at `from`; returns the state it leaves through
    uint32_t emit(const std::vector<RegexNode>& nodes, int n, uint32_t from) {
        if (overflow) return 0;
        const RegexNode& nd = nodes[n];
        switch (nd.kind) {
        case RegexNode::EMPTY: return from;
        case RegexNode::SET: {
            const uint32_t to = fresh();
            st[from].set = (int)sets.size();
            st[from].to = to;
            sets.push_back(nd.set);
            return to;
        }
        case RegexNode::CAT: {
            uint32_t cur = from;
            for (int k : nd.kids) { const uint32_t in = fresh(); st[cur].eps.push_back(in); cur = emit(nodes, k, in); if (overflow) return 0; }
            return cur;
        }
        case RegexNode::ALT: {
            const uint32_t out = fresh();
            for (int k : nd.kids) {
                const uint32_t in = fresh();
                st[from].eps.push_back(in);
                const uint32_t e = emit(nodes, k, in);
                if (overflow) return 0;
                st[e].eps.push_back(out);
            }
            return out;
        }
        case RegexNode::REPEAT: {
            uint32_t cur = from;
            for (uint32_t i = 0; i < nd.lo; ++i) { const uint32_t in = fresh(); st[cur].eps.push_back(in); cur = emit(nodes, nd.kids[0], in); if (overflow) return 0; }
            if (nd.hi == UINT32_MAX) {
                const uint32_t in = fresh(), out = fresh();
                st[cur].eps.push_back(in);
                st[cur].eps.push_back(out);
                const uint32_t e = emit(nodes, nd.kids[0], in);
                if (overflow) return 0;
                st[e].eps.push_back(in);
                st[e].eps.push_back(out);
                return out;
            }
            const uint32_t out = fresh();
            for (uint32_t i = nd.lo; i < nd.hi; ++i) {
                st[cur].eps.push_back(out);
                const uint32_t in = fresh();
                st[cur].eps.push_back(in);
                cur = emit(nodes, nd.kids[0], in);
                if (overflow) return 0;
            }
            st[cur].eps.push_back(out);
            return out;
        }
        }
        return from;
    }
};

// ----------------------------------------------------------------------------- DFA of one pattern, canonical
struct PatternDfa {
    std::vector<uint16_t> next;         // [S][256]
    std::vector<uint8_t> accepting;
};

struct RegexKeyHash {
    size_t operator()(const std::vector<int32_t>& k) const {
        uint64_t h = 0xCBF29CE484222325ull;
        for (int32_t x : k) h = (h ^ (uint32_t)x) * 0x100000001B3ull;
        return (size_t)(h ^ (h >> 29));
    }
};

// trims, minimises and renumbers a DFA given as next[S][256] (int32, -1: none), accepting, start.  probe: one byte of every class of
// bytes that no state tells apart, which is all that the refinement has to look at.  false: the language is empty
inline bool regex_canonical(std::vector<int32_t>& next, std::vector<uint8_t>& acc, uint32_t start, const std::vector<uint32_t>& probe, PatternDfa& out) {
    uint32_t S = (uint32_t)acc.size();
    // trim: keep the states that reach an accepting state (every state is reachable from the start by construction)
    std::vector<std::vector<uint32_t>> rev(S);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t b = 0; b < 256; ++b)
            if (next[(size_t)s * 256 + b] >= 0 && (b == 0 || next[(size_t)s * 256 + b] != next[(size_t)s * 256 + b - 1])) rev[next[(size_t)s * 256 + b]].push_back(s);
    std::vector<uint8_t> live(S, 0);
    std::vector<uint32_t> stack;
    for (uint32_t s = 0; s < S; ++s) if (acc[s]) { live[s] = 1; stack.push_back(s); }
    while (!stack.empty()) {
        const uint32_t s = stack.back();
        stack.pop_back();
        for (uint32_t r : rev[s]) if (!live[r]) { live[r] = 1; stack.push_back(r); }
    }
    if (!live[start]) return false;
    // Moore: block[s], refined by (block, blocks of the successors) until the number of blocks stops growing; dead states are block -1.
    // One round per step that a difference travels backwards: a chain of n states takes n rounds of n keys
    std::vector<int32_t> block(S, -1);
    for (uint32_t s = 0; s < S; ++s) if (live[s]) block[s] = acc[s] ? 1 : 0;
    size_t blocks = 0;
    for (;;) {
        std::unordered_map<std::vector<int32_t>, int32_t, RegexKeyHash> ids;
        std::vector<int32_t> nb(S, -1), key(1 + probe.size());
        for (uint32_t s = 0; s < S; ++s) {
            if (!live[s]) continue;
            key[0] = block[s];
            for (size_t c = 0; c < probe.size(); ++c) { const int32_t t = next[(size_t)s * 256 + probe[c]]; key[1 + c] = t < 0 ? -1 : block[t]; }
            nb[s] = ids.emplace(key, (int32_t)ids.size()).first->second;
        }
        block.swap(nb);
        if (ids.size() == blocks) break;
        blocks = ids.size();
    }
    // breadth-first numbering of the blocks from the start's, successors in byte order
    std::vector<uint32_t> rep(blocks, UINT32_MAX);
    for (uint32_t s = 0; s < S; ++s) if (live[s] && rep[block[s]] == UINT32_MAX) rep[block[s]] = s;
    std::vector<int32_t> num(blocks, -1);
    std::vector<uint32_t> order;
    num[block[start]] = 0;
    order.push_back((uint32_t)block[start]);
    for (size_t q = 0; q < order.size(); ++q) {
        const uint32_t s = rep[order[q]];
        for (uint32_t b = 0; b < 256; ++b) {
            const int32_t t = next[(size_t)s * 256 + b];
            if (t < 0 || !live[t]) continue;
            if (num[block[t]] < 0) { num[block[t]] = (int32_t)order.size(); order.push_back((uint32_t)block[t]); }
        }
    }
    const uint32_t N = (uint32_t)order.size();
    out.next.assign((size_t)N * 256, (uint16_t)WRK_GRAMMAR_REJECT);
    out.accepting.assign(N, 0);
    for (uint32_t k = 0; k < N; ++k) {
        const uint32_t s = rep[order[k]];
        out.accepting[k] = acc[s];
        for (uint32_t b = 0; b < 256; ++b) {
            const int32_t t = next[(size_t)s * 256 + b];
            if (t >= 0 && live[t]) out.next[(size_t)k * 256 + b] = (uint16_t)num[block[t]];
        }
    }
    return true;
}

// one pattern -> its canonical DFA.  state_budget: how many states the automaton may still take
inline bool regex_pattern_dfa(const uint8_t* pat, size_t len, uint32_t state_budget, PatternDfa& out, RegexError& err) {
    RegexParser ps(pat, len);
    const int root = ps.parse();
    if (root < 0) { err = ps.err; return false; }
    RegexNfa nfa;
    const uint32_t s0 = nfa.fresh();
    const uint32_t fin = nfa.emit(ps.nodes, root, s0);
    if (nfa.overflow) { err.code = WRK_E_UNSUPPORTED; err.offset = 0; err.what = "the pattern expands to too many NFA states"; return false; }
    // byte classes: bytes that no set of the pattern tells apart
    std::vector<uint32_t> cls(256, 0);
    uint32_t ncls = 1;
    {
        std::map<ByteSet, int> seen;
        for (const ByteSet& s : nfa.sets) {
            if (!seen.emplace(s, 0).second) continue;
            std::map<std::pair<uint32_t, bool>, uint32_t> split;
            for (uint32_t b = 0; b < 256; ++b) {
                auto it = split.emplace(std::make_pair(cls[b], bs_has(s, b)), (uint32_t)split.size()).first;
                cls[b] = it->second;
            }
            ncls = (uint32_t)split.size();
        }
    }
    std::vector<uint32_t> cls_byte(ncls, 0);
    for (uint32_t b = 256; b-- > 0;) cls_byte[cls[b]] = b;
    // subset construction
    const size_t N = nfa.st.size();
    std::vector<uint32_t> mark(N, 0);
    uint32_t stamp = 0;
    auto closure = [&](std::vector<uint32_t>& set) {
        ++stamp;
        std::vector<uint32_t> stack(set);
        for (uint32_t s : set) mark[s] = stamp;
        while (!stack.empty()) {
            const uint32_t s = stack.back();
            stack.pop_back();
            for (uint32_t t : nfa.st[s].eps) if (mark[t] != stamp) { mark[t] = stamp; set.push_back(t); stack.push_back(t); }
        }
        // only the states that matter: those with a byte edge, and the final one
        std::vector<uint32_t> keep;
        for (uint32_t s : set) if (nfa.st[s].set >= 0 || s == fin) keep.push_back(s);
        std::sort(keep.begin(), keep.end());
        set.swap(keep);
    };
    std::map<std::vector<uint32_t>, uint32_t> ids;
    std::vector<std::vector<uint32_t>> sets;
    std::vector<int32_t> next;
    std::vector<uint8_t> acc;
    std::vector<uint32_t> start{s0};
    closure(start);
    ids.emplace(start, 0u);
    sets.push_back(start);
    // more subsets than the budget can still minimise below it: allow head-room, bounded
    const size_t cap = (size_t)REGEX_MAX_STATES * 4;
    for (size_t q = 0; q < sets.size(); ++q) {
        next.resize((q + 1) * 256, -1);
        const std::vector<uint32_t> cur = sets[q];
        acc.push_back(std::binary_search(cur.begin(), cur.end(), fin) ? 1 : 0);
        std::vector<int32_t> by_cls(ncls, -1);
        for (uint32_t c = 0; c < ncls; ++c) {
            const uint32_t b = cls_byte[c];
            std::vector<uint32_t> to;
            ++stamp;
            for (uint32_t s : cur)
                if (nfa.st[s].set >= 0 && bs_has(nfa.sets[nfa.st[s].set], b) && mark[nfa.st[s].to] != stamp) { mark[nfa.st[s].to] = stamp; to.push_back(nfa.st[s].to); }
            if (to.empty()) continue;
            closure(to);
            auto it = ids.find(to);
            if (it == ids.end()) {
                if (sets.size() >= cap) { err.code = WRK_E_UNSUPPORTED; err.offset = 0; err.what = "more than 65534 automaton states"; return false; }
                it = ids.emplace(to, (uint32_t)sets.size()).first;
                sets.push_back(to);
            }
            by_cls[c] = (int32_t)it->second;
        }
        for (uint32_t b = 0; b < 256; ++b) next[q * 256 + b] = by_cls[cls[b]];
    }
    if (!regex_canonical(next, acc, 0, cls_byte, out)) { err.code = WRK_E_ARG; err.offset = 0; err.what = "the pattern matches nothing"; return false; }
    if (out.accepting.size() > state_budget) { err.code = WRK_E_UNSUPPORTED; err.offset = 0; err.what = "more than 65534 automaton states"; return false; }
    return true;
}

// several patterns -> one automaton with disjoint state sets, concatenated in pattern order.  WRK_OK, or the code with `msg` set
inline int32_t regex_compile(const char* const* patterns, const size_t* lengths, uint32_t num_patterns, wrk_byte_dfa& out, std::string& msg) {
    out = wrk_byte_dfa();
    if (!patterns || !lengths || num_patterns == 0) { msg = "patterns, lengths and at least one pattern are required"; return WRK_E_ARG; }
    for (uint32_t p = 0; p < num_patterns; ++p) {
        if (!patterns[p]) { msg = "pattern " + std::to_string(p) + ": NULL"; return WRK_E_ARG; }
        PatternDfa d;
        RegexError err;
        if (!regex_pattern_dfa((const uint8_t*)patterns[p], lengths[p], REGEX_MAX_STATES - out.num_states, d, err)) { msg = err.text(p); return err.code; }
        const uint32_t base = out.num_states, n = (uint32_t)d.accepting.size();
        out.starts.push_back(base);
        for (uint16_t t : d.next) out.next.push_back(t == WRK_GRAMMAR_REJECT ? t : (uint16_t)(t + base));
        out.accepting.insert(out.accepting.end(), d.accepting.begin(), d.accepting.end());
        out.num_states = base + n;
    }
    return WRK_OK;
}

// the same object from caller arrays: ranges are checked, nothing else
inline int32_t byte_dfa_from_arrays(uint32_t num_states, const uint16_t* next, const uint8_t* accepting, const uint32_t* starts, uint32_t num_patterns,
                                    wrk_byte_dfa& out) {
    if (!next || !accepting || !starts || num_patterns == 0 || num_states == 0 || num_states > REGEX_MAX_STATES) return WRK_E_ARG;
    for (size_t i = 0; i < (size_t)num_states * 256; ++i)
        if (next[i] >= num_states && next[i] != WRK_GRAMMAR_REJECT) return WRK_E_ARG;
    for (uint32_t p = 0; p < num_patterns; ++p) if (starts[p] >= num_states) return WRK_E_ARG;
    out.num_states = num_states;
    out.next.assign(next, next + (size_t)num_states * 256);
    out.accepting.resize(num_states);
    for (uint32_t s = 0; s < num_states; ++s) out.accepting[s] = accepting[s] != 0;
    out.starts.assign(starts, starts + num_patterns);
    return WRK_OK;
}

// bytes with identical columns of next[S][256] share a byte class, numbered by first byte.  Returns the number of classes and fills
// byte_class[256] and table[S][BC]
inline uint32_t byte_dfa_compress(const wrk_byte_dfa& d, uint8_t* byte_class, std::vector<uint16_t>& table) {
    const uint32_t S = d.num_states;
    std::map<std::vector<uint16_t>, uint32_t> ids;
    std::vector<uint32_t> first;
    std::vector<uint16_t> col(S);
    for (uint32_t b = 0; b < 256; ++b) {
        for (uint32_t s = 0; s < S; ++s) col[s] = d.next[(size_t)s * 256 + b];
        auto it = ids.emplace(col, (uint32_t)ids.size());
        if (it.second) first.push_back(b);
        byte_class[b] = (uint8_t)it.first->second;
    }
    const uint32_t BC = (uint32_t)first.size();
    table.resize((size_t)S * BC);
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t c = 0; c < BC; ++c) table[(size_t)s * BC + c] = d.next[(size_t)s * 256 + first[c]];
    return BC;
}

// ----------------------------------------------------------------------------- token classes from column hashes, exactly
// Tokens with equal 64-bit column hashes form a group whose first token represents it.  verify(token_class [V], reps, bad) walks the
// representatives and then every token against its representative's column and returns in `bad` the tokens (ascending) whose column
// differs: two columns had one hash.  Those tokens leave their group: among them, equal (old class, hash) pairs form new groups, the
// first token again the representative, and the check repeats -- each round settles at least one new representative, so it ends.
// On return classes are numbered by first token id.  WRK_OK; WRK_E_UNSUPPORTED: more than max_classes groups (reps.size() says how
// many); any other code: what verify returned.
template <class Verify>
inline int32_t group_token_classes(const uint64_t* hash, uint32_t V, uint32_t max_classes, std::vector<uint32_t>& token_class,
                                   std::vector<uint32_t>& reps, Verify verify, uint32_t* rounds_out = nullptr) {
    token_class.assign(V, 0);
    reps.clear();
    {
        std::unordered_map<uint64_t, uint32_t> ids;
        ids.reserve(1024);
        for (uint32_t t = 0; t < V; ++t) {
            auto it = ids.emplace(hash[t], (uint32_t)reps.size());
            if (it.second) reps.push_back(t);
            token_class[t] = it.first->second;
        }
    }
    uint32_t rounds = 0;
    for (;; ++rounds) {
        if (rounds_out) *rounds_out = rounds;
        if (reps.size() > max_classes) return WRK_E_UNSUPPORTED;
        std::vector<uint32_t> bad;
        const int32_t rc = verify(token_class, reps, bad);
        if (rc != WRK_OK) return rc;
        if (bad.empty()) break;
        std::map<std::pair<uint32_t, uint64_t>, uint32_t> ids;
        for (uint32_t t : bad) {
            auto it = ids.emplace(std::make_pair(token_class[t], hash[t]), (uint32_t)reps.size());
            if (it.second) reps.push_back(t);
            token_class[t] = it.first->second;
        }
    }
    // by first token id: a representative is the smallest id of its group
    std::vector<uint32_t> order(reps.size()), rank(reps.size());
    for (uint32_t c = 0; c < order.size(); ++c) order[c] = c;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return reps[a] < reps[b]; });
    std::vector<uint32_t> sorted(reps.size());
    for (uint32_t k = 0; k < order.size(); ++k) { rank[order[k]] = k; sorted[k] = reps[order[k]]; }
    reps.swap(sorted);
    for (uint32_t t = 0; t < V; ++t) token_class[t] = rank[token_class[t]];
    return WRK_OK;
}

// ----------------------------------------------------------------------------- the token-level trim and the final tables
// walk [S + 1][C]: the columns of the C representatives over the S byte-DFA states and FINAL (row S), entries < S + 1 or REJECT.
// Keeps the states from which FINAL is reachable (one backward search: every state on a path to FINAL is kept with it), turns
// transitions into dropped states into REJECT, renumbers compactly (FINAL last), merges the columns that are then equal and numbers
// the classes by first token id (the columns arrive in that order).  keep_out[s]: the new number of state s or UINT32_MAX.
inline void token_trim(uint32_t S, uint32_t C, const std::vector<uint16_t>& walk, std::vector<uint32_t>& token_class, std::vector<uint16_t>& transitions, uint32_t& num_states, uint32_t& num_classes, std::vector<uint32_t>& keep_out) {
    const uint32_t N = S + 1;
    std::vector<std::vector<uint32_t>> rev(N);
    for (uint32_t s = 0; s < N; ++s) {
        std::vector<uint16_t> row(walk.begin() + (size_t)s * C, walk.begin() + (size_t)(s + 1) * C);
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        for (uint16_t t : row) if (t != WRK_GRAMMAR_REJECT) rev[t].push_back(s);
    }
    std::vector<uint8_t> live(N, 0);
    std::vector<uint32_t> stack{S};
    live[S] = 1;
    while (!stack.empty()) {
        const uint32_t s = stack.back();
        stack.pop_back();
        for (uint32_t r : rev[s]) if (!live[r]) { live[r] = 1; stack.push_back(r); }
    }
    keep_out.assign(N, UINT32_MAX);
    num_states = 0;
    for (uint32_t s = 0; s < N; ++s) if (live[s]) keep_out[s] = num_states++;
    // columns over the kept states; equal ones merge.  reps ascend, so first occurrence is first token id
    std::map<std::vector<uint16_t>, uint32_t> ids;
    std::vector<uint32_t> merged(C);
    std::vector<std::vector<uint16_t>> cols;
    std::vector<uint16_t> col(num_states);
    for (uint32_t c = 0; c < C; ++c) {
        for (uint32_t s = 0; s < N; ++s) {
            if (!live[s]) continue;
            const uint16_t t = walk[(size_t)s * C + c];
            col[keep_out[s]] = (t == WRK_GRAMMAR_REJECT || !live[t]) ? (uint16_t)WRK_GRAMMAR_REJECT : (uint16_t)keep_out[t];
        }
        auto it = ids.emplace(col, (uint32_t)cols.size());
        if (it.second) cols.push_back(col);
        merged[c] = it.first->second;
    }
    num_classes = (uint32_t)cols.size();
    transitions.resize((size_t)num_states * num_classes);
    for (uint32_t c = 0; c < num_classes; ++c)
        for (uint32_t s = 0; s < num_states; ++s) transitions[(size_t)s * num_classes + c] = cols[c][s];
    for (uint32_t& c : token_class) c = merged[c];
}

}  // namespace wrk
