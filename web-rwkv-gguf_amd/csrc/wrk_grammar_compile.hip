// Byte DFA x vocabulary -> token automaton (wrk_grammar) for gfx950: include/wrk_hip.h wrk_grammar_compile, DESIGN.md §7v.
//
// For every automaton state s (the S byte-DFA states and FINAL = S) and every token t the walk finds where t's bytes lead:
//   r(s, t) = REJECT                          if t is empty, or a byte transition is missing on the way, or s == FINAL and t != end
//           = FINAL if accepting[s] else REJECT   if t == end_token (its bytes are ignored); FINAL for s == FINAL
//           = the state after the last byte   otherwise
// The table [S + 1][V] is never stored.  Three passes of one kernel body over (token tile, state tile) workgroups:
//   HASH    every token: h[t] = sum over s of mix(seed, s, r(s, t)) mod 2^64 (REJECT adds nothing) -- a commutative sum, so state tiles
//           add their parts with a vector atomic and the value does not depend on the order
//   FILL    the C representatives the host picked (first token of every hash group): walk[s][c] = r(s, reps[c])
//   VERIFY  every token: bad[t] = 1 where r(s, t) != walk[s][class[t]] for some s -- the host then splits the group (wrk_regex.h
//           group_token_classes), so equal hashes of different columns never reach the result
// Lanes run over tokens: a lane loads its token's bytes once (already mapped to byte classes by the host), keeps up to 16 of them in
// four registers, and reuses them for every state of the tile; its hash part stays in the lane, nothing crosses lanes.  All lanes of a
// wave start a walk in the same state, so the first look-up reads one table row (equal addresses broadcast); a walk stops at the first
// REJECT.  The table next[S][BC] (u16) is staged in LDS when it is at most 64 KiB -- two workgroups then share a CU's 160 KiB -- and read
// through L2 otherwise.  Plain vector loads and stores and one vector atomic add; no kernel waits on another.
#include <chrono>
#include <new>

#include "wrk_internal.h"
#include "wrk_regex.h"

namespace wrk {

static constexpr uint32_t GC_THREADS = 256;
static constexpr uint32_t GC_REG_BYTES = 16;                // a token of at most this many bytes stays in registers
static constexpr uint32_t GC_LDS_BYTES = 64 * 1024;         // the largest table a workgroup stages
static constexpr uint32_t GC_MIN_STATES = 32;               // states per tile at least: what pays for staging the table
static constexpr uint32_t GC_REJ = WRK_GRAMMAR_REJECT;
enum { GC_HASH = 0, GC_FILL = 1, GC_VERIFY = 2 };

struct GcParam {
    const uint8_t* bytes;       // the vocabulary's bytes as byte classes, concatenated
    const uint64_t* off;        // [V + 1]
    const uint16_t* next;       // [S][BC], padded to a multiple of 4 bytes
    const uint8_t* accepting;   // [S]
    const uint32_t* reps;       // FILL: [C] token ids
    const uint16_t* cls;        // VERIFY: [V]
    uint16_t* walk;             // FILL writes, VERIFY reads: [S + 1][C]
    unsigned long long* hash;   // HASH: [V], zeroed
    uint32_t* bad;              // VERIFY: [V], zeroed
    uint64_t seed;
    uint32_t V, S, BC, C, end_token, states_per_tile;
};

__device__ __forceinline__ uint64_t gc_mix(uint64_t seed, uint32_t s, uint32_t r) {
    uint64_t x = seed + (((uint64_t)s << 16 | r) + 1) * 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

template <int MODE, bool LDS>
__global__ void __launch_bounds__(GC_THREADS) grammar_walk_kernel(const GcParam p) {
    extern __shared__ uint16_t lds_next[];
    const uint32_t tid = threadIdx.x;
    if (LDS) {
        const uint32_t n32 = (p.S * p.BC + 1) / 2;
        const uint32_t* src = (const uint32_t*)p.next;
        uint32_t* dst = (uint32_t*)lds_next;
        for (uint32_t i = tid; i < n32; i += GC_THREADS) dst[i] = src[i];
        __syncthreads();
    }
    const uint16_t* tab = LDS ? lds_next : p.next;
    const uint32_t n = MODE == GC_FILL ? p.C : p.V;
    const uint32_t idx = blockIdx.x * GC_THREADS + tid;
    if (idx >= n) return;
    const uint32_t t = MODE == GC_FILL ? p.reps[idx] : idx;
    const uint64_t o = p.off[t];
    const uint64_t len64 = p.off[t + 1] - o;
    const uint32_t len = len64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len64;
    const uint8_t* tb = p.bytes + o;
    uint32_t w[GC_REG_BYTES / 4] = {0u, 0u, 0u, 0u};
    if (len <= GC_REG_BYTES) {
#pragma unroll
        for (uint32_t i = 0; i < GC_REG_BYTES; ++i)
            if (i < len) w[i / 4] |= (uint32_t)tb[i] << (8 * (i % 4));
    }
    const uint32_t s0 = blockIdx.y * p.states_per_tile;
    const uint32_t s1 = min(s0 + p.states_per_tile, p.S + 1);
    const uint32_t c = MODE == GC_VERIFY ? p.cls[t] : idx;
    const bool is_end = t == p.end_token;
    uint64_t h = 0;
    bool differs = false;
    for (uint32_t s = s0; s < s1; ++s) {
        uint32_t cur;
        if (s == p.S) cur = is_end ? p.S : GC_REJ;
        else if (is_end) cur = p.accepting[s] ? p.S : GC_REJ;
        else if (len == 0) cur = GC_REJ;
        else if (len <= GC_REG_BYTES) {
            cur = s;
#pragma unroll
            for (uint32_t i = 0; i < GC_REG_BYTES; ++i) {
                if (i >= len || cur == GC_REJ) break;
                cur = tab[cur * p.BC + ((w[i / 4] >> (8 * (i % 4))) & 0xFFu)];
            }
        } else {
            cur = s;
            for (uint32_t i = 0; i < len && cur != GC_REJ; ++i) cur = tab[cur * p.BC + tb[i]];
        }
        if (MODE == GC_HASH) { if (cur != GC_REJ) h += gc_mix(p.seed, s, cur); }
        if (MODE == GC_FILL) p.walk[(size_t)s * p.C + c] = (uint16_t)cur;
        if (MODE == GC_VERIFY) differs |= p.walk[(size_t)s * p.C + c] != (uint16_t)cur;
    }
    if (MODE == GC_HASH && h != 0) atomicAdd(p.hash + t, (unsigned long long)h);
    if (MODE == GC_VERIFY && differs) p.bad[t] = 1u;
}

// how the state range [0, S] is cut: enough workgroups to fill the chip, no tile below GC_MIN_STATES states
static uint32_t gc_states_per_tile(uint32_t items, uint32_t S, uint32_t num_cu) {
    const uint32_t token_tiles = (items + GC_THREADS - 1) / GC_THREADS;
    const uint32_t want = (8 * num_cu + token_tiles - 1) / token_tiles;      // state tiles for about 8 workgroups per CU
    const uint32_t per = (S + 1 + want - 1) / want;
    return per < GC_MIN_STATES ? GC_MIN_STATES : per;
}

template <int MODE>
static void gc_launch(hipStream_t st, GcParam p, uint32_t items, uint32_t num_cu) {
    if (items == 0) return;
    p.states_per_tile = gc_states_per_tile(items, p.S, num_cu);
    const dim3 grid((items + GC_THREADS - 1) / GC_THREADS, (p.S + 1 + p.states_per_tile - 1) / p.states_per_tile);
    const size_t tab_bytes = ((size_t)p.S * p.BC * 2 + 3) & ~(size_t)3;
    if (tab_bytes <= GC_LDS_BYTES) grammar_walk_kernel<MODE, true><<<grid, GC_THREADS, tab_bytes, st>>>(p);
    else grammar_walk_kernel<MODE, false><<<grid, GC_THREADS, 0, st>>>(p);
}

static thread_local float g_compile_ms[WRK_GRAMMAR_COMPILE_PHASES];

}  // namespace wrk

namespace {
struct Clock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    float lap() {
        const auto t1 = std::chrono::steady_clock::now();
        const float ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
        t0 = t1;
        return ms;
    }
};
void put_err(char* err, size_t cap, const std::string& msg) {
    if (err && cap) snprintf(err, cap, "%s", msg.c_str());
}
}  // namespace

extern "C" {

int32_t wrk_regex_compile(const char* const* patterns, const size_t* lengths, uint32_t num_patterns, wrk_byte_dfa** out, char* err, size_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!out) return WRK_E_ARG;
    *out = nullptr;
    wrk_byte_dfa* d = new (std::nothrow) wrk_byte_dfa;
    if (!d) return WRK_E_OOM;
    std::string msg;
    int32_t rc;
    try {
        rc = wrk::regex_compile(patterns, lengths, num_patterns, *d, msg);
    } catch (const std::bad_alloc&) {
        rc = WRK_E_OOM;
        msg = "out of memory";
    }
    if (rc != WRK_OK) { delete d; put_err(err, err_cap, msg); return rc; }
    *out = d;
    return WRK_OK;
}

int32_t wrk_byte_dfa_from_arrays(uint32_t num_states, const uint16_t* next, const uint8_t* accepting, const uint32_t* starts, uint32_t num_patterns,
                                 wrk_byte_dfa** out) {
    if (!out) return WRK_E_ARG;
    *out = nullptr;
    wrk_byte_dfa* d = new (std::nothrow) wrk_byte_dfa;
    if (!d) return WRK_E_OOM;
    const int32_t rc = wrk::byte_dfa_from_arrays(num_states, next, accepting, starts, num_patterns, *d);
    if (rc != WRK_OK) { delete d; return rc; }
    *out = d;
    return WRK_OK;
}

int32_t wrk_byte_dfa_export(const wrk_byte_dfa* d, uint32_t* num_states, uint32_t* num_patterns, uint16_t* next, uint8_t* accepting, uint32_t* starts) {
    if (!d) return WRK_E_ARG;
    if (num_states) *num_states = d->num_states;
    if (num_patterns) *num_patterns = (uint32_t)d->starts.size();
    if (next) memcpy(next, d->next.data(), d->next.size() * 2);
    if (accepting) memcpy(accepting, d->accepting.data(), d->accepting.size());
    if (starts) memcpy(starts, d->starts.data(), d->starts.size() * 4);
    return WRK_OK;
}

void wrk_byte_dfa_destroy(wrk_byte_dfa* d) { delete d; }

int32_t wrk_grammar_compile(wrk_ctx* ctx, const wrk_byte_dfa* dfa, uint32_t V, const uint8_t* vocab_bytes, const uint64_t* vocab_offsets,
                            uint32_t end_token, wrk_grammar** out, uint32_t* start_states, uint32_t* final_state) {
    if (!ctx || !out) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    *out = nullptr;
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_grammar_compile is blocking: not inside a capture");
    WRK_ARG(ctx, dfa && vocab_bytes && vocab_offsets && start_states && final_state, "dfa, vocab_bytes, vocab_offsets, start_states and final_state are required");
    WRK_ARG(ctx, V >= 1, "num_vocab 0");
    if (V > wrk::SAMPLE_MAX_VOCAB) return wrk_fail(ctx, WRK_E_UNSUPPORTED, "num_vocab %u > %u", V, wrk::SAMPLE_MAX_VOCAB);
    WRK_ARG(ctx, end_token < V, "end_token %u >= num_vocab %u", end_token, V);
    for (uint32_t t = 0; t < V; ++t)
        WRK_ARG(ctx, vocab_offsets[t] <= vocab_offsets[t + 1], "vocab_offsets[%u] > vocab_offsets[%u]", t, t + 1);
    const uint32_t S = dfa->num_states, P = (uint32_t)dfa->starts.size();
    WRK_ARG(ctx, S >= 1 && S <= wrk::REGEX_MAX_STATES && P >= 1, "an empty byte automaton");
    for (float& ms : wrk::g_compile_ms) ms = 0.f;
    Clock clock;

    // host: byte classes, and the vocabulary's bytes mapped to them
    uint8_t byte_class[256];
    std::vector<uint16_t> table;
    const uint32_t BC = wrk::byte_dfa_compress(*dfa, byte_class, table);
    const uint64_t base = vocab_offsets[0], total = vocab_offsets[V] - base;
    std::vector<uint8_t> mapped(total);
    for (uint64_t i = 0; i < total; ++i) mapped[i] = byte_class[vocab_bytes[base + i]];
    std::vector<uint64_t> off(V + 1);
    for (uint32_t t = 0; t <= V; ++t) off[t] = vocab_offsets[t] - base;
    table.resize((table.size() + 1) & ~(size_t)1, (uint16_t)WRK_GRAMMAR_REJECT);      // whole dwords for the LDS staging
    wrk::g_compile_ms[0] = clock.lap();

    WRK_HIP(ctx, hipSetDevice(ctx->device));
    wrk_dev_arena dev;
    const size_t o_bytes = dev.add(total), o_off = dev.add((size_t)(V + 1) * 8), o_next = dev.add(table.size() * 2), o_acc = dev.add(S),
                 o_hash = dev.add((size_t)V * 8), o_cls = dev.add((size_t)V * 2), o_bad = dev.add((size_t)V * 4);
    WRK_HIP(ctx, dev.alloc());
    hipStream_t st = ctx->stream;
    if (total) WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_bytes), mapped.data(), total, hipMemcpyHostToDevice, st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_off), off.data(), (size_t)(V + 1) * 8, hipMemcpyHostToDevice, st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_next), table.data(), table.size() * 2, hipMemcpyHostToDevice, st));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_acc), dfa->accepting.data(), S, hipMemcpyHostToDevice, st));
    WRK_HIP(ctx, hipMemsetAsync(dev.at<char>(o_hash), 0, (size_t)V * 8, st));
    wrk::GcParam par{};
    par.bytes = dev.at<uint8_t>(o_bytes); par.off = dev.at<uint64_t>(o_off); par.next = dev.at<uint16_t>(o_next);
    par.accepting = dev.at<uint8_t>(o_acc); par.cls = dev.at<uint16_t>(o_cls); par.hash = dev.at<unsigned long long>(o_hash);
    par.bad = dev.at<uint32_t>(o_bad);
    par.seed = 0x243F6A8885A308D3ull;
    par.V = V; par.S = S; par.BC = BC; par.end_token = end_token;

    // pass 1: a hash per token
    wrk::gc_launch<wrk::GC_HASH>(st, par, V, (uint32_t)ctx->num_cu);
    WRK_LAUNCH_CHECK(ctx);
    std::vector<uint64_t> hash(V);
    WRK_HIP(ctx, hipMemcpyAsync(hash.data(), dev.at<char>(o_hash), (size_t)V * 8, hipMemcpyDeviceToHost, st));
    WRK_HIP(ctx, hipStreamSynchronize(st));
    wrk::g_compile_ms[1] = clock.lap();

    // passes 2 and 3 under the exact grouping
    std::vector<uint32_t> cls32, reps;
    std::vector<uint16_t> walk, cls16(V);
    wrk_dev_arena wdev;         // reps and walk, sized once the number of groups is known; regrown when a split adds groups
    size_t o_reps = 0, o_walk = 0;
    uint32_t cap = 0;
    float ms_fill = 0.f, ms_verify = 0.f;
    auto verify = [&](const std::vector<uint32_t>& tc, const std::vector<uint32_t>& rp, std::vector<uint32_t>& bad) -> int32_t {
        const uint32_t C = (uint32_t)rp.size();
        Clock c2;
        if (C > cap) {
            if (wdev.base) { WRK_HIP(ctx, hipFree(wdev.base)); wdev.base = nullptr; wdev.total = 0; }
            cap = C;
            o_reps = wdev.add((size_t)cap * 4);
            o_walk = wdev.add((size_t)(S + 1) * cap * 2);
            WRK_HIP(ctx, wdev.alloc());
        }
        for (uint32_t t = 0; t < V; ++t) cls16[t] = (uint16_t)tc[t];
        WRK_HIP(ctx, hipMemcpyAsync(wdev.at<char>(o_reps), rp.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
        WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_cls), cls16.data(), (size_t)V * 2, hipMemcpyHostToDevice, st));
        WRK_HIP(ctx, hipMemsetAsync(dev.at<char>(o_bad), 0, (size_t)V * 4, st));
        par.reps = wdev.at<uint32_t>(o_reps); par.walk = wdev.at<uint16_t>(o_walk); par.C = C;
        wrk::gc_launch<wrk::GC_FILL>(st, par, C, (uint32_t)ctx->num_cu);
        WRK_LAUNCH_CHECK(ctx);
        WRK_HIP(ctx, hipStreamSynchronize(st));
        ms_fill += c2.lap();
        wrk::gc_launch<wrk::GC_VERIFY>(st, par, V, (uint32_t)ctx->num_cu);
        WRK_LAUNCH_CHECK(ctx);
        std::vector<uint32_t> flags(V);
        WRK_HIP(ctx, hipMemcpyAsync(flags.data(), dev.at<char>(o_bad), (size_t)V * 4, hipMemcpyDeviceToHost, st));
        WRK_HIP(ctx, hipStreamSynchronize(st));
        for (uint32_t t = 0; t < V; ++t) if (flags[t]) bad.push_back(t);
        ms_verify += c2.lap();
        return WRK_OK;
    };
    // the class ids travel as u16: the limit holds before the walk of the representatives, which bounds the scratch by S x 8192 entries
    const int32_t grc = wrk::group_token_classes(hash.data(), V, WRK_MAX_TOKEN_CLASSES, cls32, reps, verify);
    if (grc == WRK_E_UNSUPPORTED)
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "the vocabulary has %zu distinct columns in this automaton, at most %u token classes", reps.size(),
                        (uint32_t)WRK_MAX_TOKEN_CLASSES);
    if (grc != WRK_OK) return grc;
    // the grouping renumbered the classes by first token id: the columns come back in that order with one more walk of the representatives
    const uint32_t C = (uint32_t)reps.size();
    {
        Clock c2;
        WRK_HIP(ctx, hipMemcpyAsync(wdev.at<char>(o_reps), reps.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
        par.reps = wdev.at<uint32_t>(o_reps); par.walk = wdev.at<uint16_t>(o_walk); par.C = C;
        wrk::gc_launch<wrk::GC_FILL>(st, par, C, (uint32_t)ctx->num_cu);
        WRK_LAUNCH_CHECK(ctx);
        walk.resize((size_t)(S + 1) * C);
        WRK_HIP(ctx, hipMemcpyAsync(walk.data(), wdev.at<char>(o_walk), walk.size() * 2, hipMemcpyDeviceToHost, st));
        WRK_HIP(ctx, hipStreamSynchronize(st));
        ms_fill += c2.lap();
    }
    clock.lap();
    wrk::g_compile_ms[2] = ms_fill;
    wrk::g_compile_ms[3] = ms_verify;

    // host: the token-level trim, then the ordinary constructor
    std::vector<uint16_t> transitions;
    std::vector<uint32_t> keep;
    uint32_t NS = 0, NC = 0;
    wrk::token_trim(S, C, walk, cls32, transitions, NS, NC, keep);
    for (uint32_t p = 0; p < P; ++p)
        WRK_ARG(ctx, keep[dfa->starts[p]] != UINT32_MAX, "the vocabulary cannot spell pattern %u", p);
    for (uint32_t t = 0; t < V; ++t) cls16[t] = (uint16_t)cls32[t];
    wrk::g_compile_ms[4] = clock.lap();
    const int32_t rc = wrk_grammar_create(ctx, V, NS, NC, cls16.data(), transitions.data(), out);
    if (rc != WRK_OK) return rc;
    for (uint32_t p = 0; p < P; ++p) start_states[p] = keep[dfa->starts[p]];
    *final_state = keep[S];
    wrk::g_compile_ms[5] = clock.lap();
    return WRK_OK;
}

int32_t wrk_grammar_compile_last_ms(float* ms) {
    if (!ms) return WRK_E_ARG;
    for (uint32_t i = 0; i < WRK_GRAMMAR_COMPILE_PHASES; ++i) ms[i] = wrk::g_compile_ms[i];
    return WRK_OK;
}

int32_t wrk_grammar_export(const wrk_grammar* g, uint32_t* num_states, uint32_t* num_classes, uint16_t* token_class, uint16_t* transitions) {
    if (!g) return WRK_E_ARG;
    wrk_ctx* ctx = g->ctx;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    WRK_ARG(ctx, !ctx->capturing_here(), "wrk_grammar_export is blocking: not inside a capture");
    if (num_states) *num_states = g->num_states;
    if (num_classes) *num_classes = g->num_classes;
    if (!token_class && !transitions) return WRK_OK;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    if (token_class) WRK_HIP(ctx, hipMemcpyAsync(token_class, g->token_class, (size_t)g->num_vocab * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (transitions)
        WRK_HIP(ctx, hipMemcpyAsync(transitions, g->transitions, (size_t)g->num_states * g->num_classes * 2, hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WRK_OK;
}

}  // extern "C"
