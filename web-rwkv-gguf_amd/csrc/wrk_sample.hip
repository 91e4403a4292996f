// On-device nucleus sampling for gfx950: examples/chat.rs:150-190 `Sampler::sample` (softmax, top-p cut, temperature inside the
// nucleus, inverse-CDF draw), one workgroup per row of f32 logits.  See DESIGN.md "Sampling on the device".
//
// Order: tokens by logit descending (== p descending), ties by index ascending.  That order is the 52-bit key
// K = monotone(logit) << 20 | (2^20 - 1 - index), unique per token.  Both decisions -- the nucleus boundary and the drawn token --
// are a weighted select over K, done as a radix descent with LDS histograms:
//   pass 0      digit = distance below the row max, the row's finite range cut into 2048 bins (monotone in K), which spreads a row over
//               many bins (the top bits of K are nearly constant over a row and would pile every token into a few bins);
//   passes 1-5  digits = bits [41,52), [30,41), [19,30), [8,19), [0,8) of K, among the tokens left in the chosen bins;
// each pass stops the descent as soon as the chosen bin holds one token.  Masses are fixed point (e * 2^40 in u64): every sum that
// feeds a decision is an integer sum, so the result does not depend on the order the atomics land in.
//
// MODE SAMPLE_FILT (DESIGN.md "Top-k and min-p") shares the body.  A top-k cut is one more prefix of the same order: its
// boundary, the token at rank top_k - 1, is a COUNT select over K, and the pass histograms already hold cnt next to mass, so it rides the
// nucleus's descent: each pass finds the bin the mass target chooses and the bin the count target chooses; the higher bin (the earlier
// rank) wins and the other target is dropped, equal bins descend with both.  The min-p cut, fl32(l - mx) >= ln(min_p), is part of the
// draw's candidate predicate.
//
// MODE SAMPLE_MIRO and SAMPLE_TYP (DESIGN.md "Mirostat v2 and locally typical sampling") share the body too.
// Mirostat: one full-row mass pass gives W; "rank 0, or surprise <= mu" is a term of the draw's candidate predicate; no boundary descent;
// the draw's pass-0 total is W_c, from which one lane takes the drawn token's surprise and writes the next mu.  Typical: one moments
// pass (sum e and sum e g in fixed point, g = max - l) gives gbar; the boundary is the nucleus's mass select over the key
// monotone(-d) << 20 | (2^20 - 1 - index), d = |g - gbar|, with the pass-0 digit taken from the range of d; the draw's candidates are
// the tokens whose d-key is >= the boundary's.  The descent is one lambda, generic in which key it walks.
//
// MODE SAMPLE_CUT (DESIGN.md "XTC, top-n-sigma and the eta / epsilon cut-offs") is SAMPLE_FILT's body with two additions.  Upper end: the
// three new cuts are, like min-p, lower bounds on d = l - max, so the draw's predicate keeps its one compare, against
//   thr = max(ln_min_p, -top_n_sigma * sigma, ln_epsilon + ln S, min(ln_eta, ln_eta / 2 - H) + ln S),
// rank 0 always in.  S = sum e and H = ln S + gbar come from the typical kernel's moments pass (fixed point); sigma from one pass of
// integer moments of q = trunc((max - l) * 2^21 / (max - low)) over the finite logits: sigma = sqrt(N sum q^2 - (sum q)^2) / N in units of
// (max - low) / 2^21, the radicand an exact 128-bit integer.  Lower end (XTC): the row's coin c = (sample_splitmix_next >> 40) * 2^-24,
// the second output of the SplitMix64 stream whose first gives u; with c < xtc_probability one count / min-key pass over the candidates
// with d >= ln(xtc_threshold) + ln S gives m' and the key of rank m' - 1, and with m' >= 2 the draw runs on kmin <= K <= kmax, its
// weights exp((l - l_m0) / T) relative to the logit of rank m0 = m' - 1, read back out of that key.  A pass a
// row's parameters do not ask for is skipped; every sum is an integer sum and the minimum is a minimum of unique keys.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "wrk_rows_dev.h"

namespace wrk {

static constexpr uint32_t SAMPLE_BINS = 2048;
static constexpr uint32_t SAMPLE_THREADS = 1024;
static constexpr float SAMPLE_ONE = 1099511627776.0f;      // 2^40: mass of the row's top token

__host__ __device__ inline uint64_t sample_splitmix(uint32_t seed, uint32_t step) {
    uint64_t z = (((uint64_t)seed << 32) | step) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the second output of the SplitMix64 stream whose first output is sample_splitmix(seed, step): the state advanced once more
__host__ __device__ inline uint64_t sample_splitmix_next(uint32_t seed, uint32_t step) {
    uint64_t z = (((uint64_t)seed << 32) | step) + 2ull * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// pass-0 digit, higher = earlier rank: (mx - l) * scale, monotone in l; l == mx also covers mx = +inf
__device__ __forceinline__ uint32_t coarse_digit(float l, float mx, float scale) {
    const float d = l == mx ? 0.0f : (mx - l) * scale;
    return (SAMPLE_BINS - 1) - (uint32_t)fminf(d, (float)(SAMPLE_BINS - 1));
}

// typical order: d = |(mx - l) - gbar| ascending, ties by index ascending; d >= 0 or +inf (a -inf logit), never NaN
__device__ __forceinline__ float typical_dist(float l, float mx, float gbar) { return fabsf((l == mx ? 0.0f : mx - l) - gbar); }
__device__ __forceinline__ uint64_t typical_key(float d, uint32_t i) {
    return ((uint64_t)(0x7FFFFFFFu - __float_as_uint(d)) << 20) | (0xFFFFFu - i);     // monotone(-d) of a d >= 0
}
__device__ __forceinline__ uint32_t typical_digit(float d, float scale) {
    return (SAMPLE_BINS - 1) - (uint32_t)fminf(d * scale, (float)(SAMPLE_BINS - 1));
}

static constexpr float SAMPLE_LOG2E = 1.44269504088896340736f;
static constexpr float SAMPLE_LN_ONE = 27.725887222397812f;     // ln 2^40
static constexpr float SAMPLE_SIGMA_ONE = 2097152.0f;            // 2^21: the fixed point of (max - l) / (max - low)

struct SampleSmem {
    unsigned long long mass[SAMPLE_BINS];
    uint32_t cnt[SAMPLE_BINS];
    uint32_t idx[SAMPLE_BINS];
    unsigned long long wsum[SAMPLE_THREADS / WAVE];
    float wmax[SAMPLE_THREADS / WAVE], wmin[SAMPLE_THREADS / WAVE];
    uint32_t widx[SAMPLE_THREADS / WAVE];
    unsigned long long sel_above;
    uint32_t sel, sel_cnt, sel_idx;
    uint32_t wcnt[SAMPLE_THREADS / WAVE], selk, sel_cabove;     // filtered kernel: the count select next to the mass select
};

// exclusive prefix of v over the workgroup in thread order; *total = the sum (same value in every thread)
__device__ __forceinline__ unsigned long long block_excl_scan(unsigned long long v, SampleSmem& sm, unsigned long long* total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(x, o, WAVE);
        if (lane >= (uint32_t)o) x += t;
    }
    if (lane == 63) sm.wsum[wid] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SAMPLE_THREADS / WAVE; ++w) {
        const unsigned long long s = sm.wsum[w];
        if (w < wid) before += s;
        all += s;
    }
    *total = all;
    return before + x - v;
}

// block_excl_scan of v and of c in one go; *cbefore = the exclusive prefix of c
__device__ __forceinline__ unsigned long long block_excl_scan2(unsigned long long v, uint32_t c, SampleSmem& sm, unsigned long long* total,
                                                               uint32_t* cbefore) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long x = v;
    uint32_t y = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(x, o, WAVE);
        const uint32_t u = __shfl_up(y, o, WAVE);
        if (lane >= (uint32_t)o) { x += t; y += u; }
    }
    if (lane == 63) { sm.wsum[wid] = x; sm.wcnt[wid] = y; }
    __syncthreads();
    unsigned long long before = 0, all = 0;
    uint32_t cb = 0;
#pragma unroll
    for (uint32_t w = 0; w < SAMPLE_THREADS / WAVE; ++w) {
        const unsigned long long s = sm.wsum[w];
        if (w < wid) { before += s; cb += sm.wcnt[w]; }
        all += s;
    }
    *total = all;
    *cbefore = cb + y - c;
    return before + x - v;
}

// sum of v over the workgroup (same value in every thread); an integer sum: independent of the order
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, SampleSmem& sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    __syncthreads();            // the readers of an earlier wsum are done
    if ((threadIdx.x & 63) == 0) sm.wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SAMPLE_THREADS / WAVE; ++w) all += sm.wsum[w];
    return all;
}

// minimum of v over the workgroup (same value in every thread)
__device__ __forceinline__ unsigned long long block_min(unsigned long long v, SampleSmem& sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, WAVE);
        v = t < v ? t : v;
    }
    __syncthreads();            // the readers of an earlier wsum are done
    if ((threadIdx.x & 63) == 0) sm.wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long all = ~0ull;
#pragma unroll
    for (uint32_t w = 0; w < SAMPLE_THREADS / WAVE; ++w) all = sm.wsum[w] < all ? sm.wsum[w] : all;
    return all;
}

static constexpr uint32_t SAMPLE_NO_COUNT = 0xffffffffu;

// One row per workgroup.  NPT > 0: the row (V <= 1024 * NPT) stays in registers; NPT == 0: every pass re-reads it from L2 (V <= 2^20;
// a 64-per-thread register copy of a 65536-token row spills, the passes' own state needs ~95 VGPRs)
// MODE SAMPLE_FILT: the filtered kernel's body (filt: one SampleFilter per row); every addition sits under `if constexpr (FILT)`.
// SAMPLE_MIRO / SAMPLE_TYP: the Mirostat / typical kernel's (alt: one SampleAlt per row); additions under `if constexpr (MIRO)` / `(TYP)`
// SAMPLE_CUT: the filtered kernel's body (FILT holds) and the cuts of cut[row]; every addition sits under `if constexpr (CUT)`
template <int NPT, int MODE>
__device__ __forceinline__ void sample_rows_body(SampleSmem& sm, const float* __restrict__ logits, uint32_t V, uint32_t stride,
                                                 const SampleParam* __restrict__ par, const SampleFilter* __restrict__ filt,
                                                 SampleAlt* alt, const RowGate gate,
                                                 const uint32_t* __restrict__ step_word, uint32_t* __restrict__ out,
                                                 const SampleCut* __restrict__ cut) {
    constexpr bool CUT = MODE == SAMPLE_CUT, FILT = MODE == SAMPLE_FILT || CUT, MIRO = MODE == SAMPLE_MIRO, TYP = MODE == SAMPLE_TYP;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = logits + (size_t)blockIdx.x * stride;
    const int nj = NPT > 0 ? NPT : (int)((V + SAMPLE_THREADS - 1) / SAMPLE_THREADS);
    auto load = [&](int j) -> float {
        const uint32_t i = tid + SAMPLE_THREADS * (uint32_t)j;
        const float x = i < V ? row[i] : -INFINITY;
        return row_norm(x);
    };
    float lv[NPT > 0 ? NPT : 1];
    if constexpr (NPT > 0) {
#pragma unroll
        for (int j = 0; j < NPT; ++j) lv[j] = load(j);
    }
    // f(j, logit) over this thread's elements; from memory, 16 loads are issued ahead of their use (one at a time, every pass would pay the
    // L2 latency 64 times over)
    auto for_each = [&](auto&& f) __attribute__((always_inline)) {
        if constexpr (NPT > 0) {
#pragma unroll
            for (int j = 0; j < NPT; ++j) f(j, lv[j]);
        } else {
            for (int j0 = 0; j0 < nj; j0 += 16) {
                float c[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) c[u] = load(j0 + u);      // past the row: -inf, and i >= V for every test below
#pragma unroll
                for (int u = 0; u < 16; ++u) f(j0 + u, c[u]);
            }
        }
    };

    // row max and the first index holding it (argmax_rows' answer whenever the max exceeds -3e38)
    float best = -INFINITY, low = INFINITY;        // low: the smallest logit above -inf
    uint32_t bi = 0xffffffffu;
    for_each([&](int j, float x) {
        if (x > best) { best = x; bi = tid + SAMPLE_THREADS * (uint32_t)j; }
        if (x > -INFINITY) low = fminf(low, x);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, WAVE);
        const uint32_t oi = __shfl_xor(bi, o, WAVE);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        low = fminf(low, __shfl_xor(low, o, WAVE));
    }
    if (lane == 0) { sm.wmax[wid] = best; sm.widx[wid] = bi; sm.wmin[wid] = low; }
    __syncthreads();
    best = sm.wmax[0]; bi = sm.widx[0]; low = sm.wmin[0];
    for (uint32_t w = 1; w < SAMPLE_THREADS / WAVE; ++w) {
        if (sm.wmax[w] > best || (sm.wmax[w] == best && sm.widx[w] < bi)) { best = sm.wmax[w]; bi = sm.widx[w]; }
        low = fminf(low, sm.wmin[w]);
    }
    const float mx = best;
    const uint32_t top = bi;
    // pass-0 bins span the row's finite range, so that a row whose logits lie close together (a flat distribution) still spreads over the
    // bins instead of piling into a few and serialising their atomics; the digit only has to be monotone in l
    const float span = (mx - low) * (1.0f / (float)(SAMPLE_BINS - 1));
    float scale = 1.0f / span;
    if (!(scale > 0.0f) || !(scale < INFINITY)) scale = 64.0f;

    const SampleParam pr = par[blockIdx.x];
    const float temp = pr.temperature;
    float top_p = pr.top_p;
    bool miro = false, typ = false;     // the row's own sampler is on (off: a plain sampler row)
    float tau = 0.0f, eta = 0.0f, mu = 0.0f, typical_p = 1.0f;
    if constexpr (MIRO || TYP) {
        const SampleAlt a = alt[blockIdx.x];
        tau = a.tau; eta = a.eta; mu = a.mu; typical_p = a.typical_p;
        miro = MIRO && tau > 0.0f;
        typ = TYP && !(typical_p >= 1.0f);
        if (miro || typ) top_p = 1.0f;      // not read by such a row: neither its greedy test nor a nucleus cut
    }
    uint32_t top_k = 0;             // 0: no top-k cut (top_k >= V cuts nothing either)
    float ln_min_p = -INFINITY;
    if constexpr (FILT) {
        const SampleFilter fl = filt[blockIdx.x];
        top_k = fl.top_k >= V ? 0u : fl.top_k;
        ln_min_p = fl.ln_min_p;
    }
    if (!(temp > 0.0f) || !(top_p > 0.0f) || mx == -INFINITY || (FILT && top_k == 1)) {       // greedy: bit-identical to argmax_rows
        if (tid == 0) out[blockIdx.x] = mx > -3.0e38f ? top : 0u;
        return;
    }
    const float inv_t = 1.0f / temp;

    // Mirostat: W in fixed point over the whole row -> log2 W; a token is a candidate iff it is rank 0 or its surprise is <= mu
    float log2_w = 0.0f;
    if constexpr (MIRO) {
        if (miro) {
            unsigned long long acc = 0;
            for_each([&](int j, float l) {
                if (tid + SAMPLE_THREADS * (uint32_t)j < V) acc += (unsigned long long)((l == mx ? 1.0f : expf((l - mx) * inv_t)) * SAMPLE_ONE);
            });
            log2_w = log2f((float)block_sum(acc, sm)) - 40.0f;
        }
    }
    // typical: gbar = sum e g / sum e with e = exp(l - mx), g = mx - l, both sums in fixed point (e g <= 1 / e: no overflow below 2^20 tokens);
    // a -inf logit adds nothing to either.  The pass-0 digit of the d-key spreads [0, max d] over the bins
    float gbar = 0.0f, dscale = 64.0f;
    if constexpr (TYP) {
        if (typ) {
            unsigned long long se = 0, seg = 0;
            for_each([&](int j, float l) {      // branch-free: two accumulators updated under different branches end up in scratch
                const bool in = tid + SAMPLE_THREADS * (uint32_t)j < V && l > -INFINITY;
                const float g = l == mx ? 0.0f : mx - l, e = l == mx ? 1.0f : expf(l - mx);
                const float eg = in && e > 0.0f ? e * g : 0.0f;     // mx = +inf: g = inf next to e = 0
                se += in ? (unsigned long long)(e * SAMPLE_ONE) : 0ull;
                seg += (unsigned long long)(eg * SAMPLE_ONE);
            });
            se = block_sum(se, sm);
            seg = block_sum(seg, sm);
            gbar = (float)((double)seg / (double)se);
            const float dmax = fmaxf(gbar, (mx - low) - gbar);      // low: the smallest finite logit (mx = +inf: inf, the scale falls back)
            dscale = (float)(SAMPLE_BINS - 1) / dmax;
            if (!(dscale > 0.0f) || !(dscale < INFINITY)) dscale = 64.0f;
        }
    }
    unsigned long long draw_total = 0;      // Mirostat: W_c, the draw's pass-0 total
    // cut rows.  thr: the lowest d = l - max of a candidate below rank 0 (min-p, top-n-sigma, epsilon and eta in one bound; all four
    // off: ln_min_p, SAMPLE_FILT's test).  xtc: the coin fell below xtc_probability; thr_x: the d of xtc_threshold
    float thr = ln_min_p, thr_x = 0.0f;
    bool xtc = false;
    if constexpr (CUT) {
        const SampleCut ct = cut[blockIdx.x];
        const float coin = (float)(sample_splitmix_next(pr.seed, *step_word - pr.step_base) >> 40) * 5.9604644775390625e-8f;     // * 2^-24: exact
        xtc = coin < ct.xtc_probability;
        const bool use_h = ct.ln_eta > -INFINITY, use_e = ct.ln_epsilon > -INFINITY;
        if (use_h || use_e || xtc) {        // the typical kernel's moments pass: S = sum e, and gbar = sum e g / sum e for H = ln S + gbar
            unsigned long long se = 0, seg = 0;
            for_each([&](int j, float l) {
                const bool in = tid + SAMPLE_THREADS * (uint32_t)j < V && l > -INFINITY;
                const float g = l == mx ? 0.0f : mx - l, e = l == mx ? 1.0f : expf(l - mx);
                const float eg = in && e > 0.0f ? e * g : 0.0f;
                se += in ? (unsigned long long)(e * SAMPLE_ONE) : 0ull;
                seg += (unsigned long long)(eg * SAMPLE_ONE);
            });
            se = block_sum(se, sm);
            seg = block_sum(seg, sm);
            const float ln_s = logf((float)se) - SAMPLE_LN_ONE;
            if (use_e) thr = fmaxf(thr, ct.ln_epsilon + ln_s);
            if (use_h) {
                const float h = ln_s + (float)((double)seg / (double)se);
                thr = fmaxf(thr, fminf(ct.ln_eta, 0.5f * ct.ln_eta - h) + ln_s);
            }
            thr_x = ct.ln_xtc_threshold + ln_s;
        }
        // sigma of the finite logits; max - low == 0, or not finite (max = +inf): sigma = 0, the ties of the maximum stay (thr <= 0 already)
        const float qs = SAMPLE_SIGMA_ONE / (mx - low);
        if (ct.top_n_sigma > 0.0f && qs > 0.0f && qs < INFINITY) {
            unsigned long long cn = 0, t1 = 0, t2 = 0;
            for_each([&](int j, float l) {
                const bool in = tid + SAMPLE_THREADS * (uint32_t)j < V && l > -INFINITY;
                const unsigned long long q = in ? (unsigned long long)fminf((mx - l) * qs, SAMPLE_SIGMA_ONE) : 0ull;
                cn += in ? 1ull : 0ull;
                t1 += q;
                t2 += q * q;            // q <= 2^21, at most 2^20 terms: below 2^62
            });
            cn = block_sum(cn, sm);
            t1 = block_sum(t1, sm);
            t2 = block_sum(t2, sm);
            const unsigned __int128 rad = (unsigned __int128)cn * t2 - (unsigned __int128)t1 * t1;      // >= 0 (Cauchy-Schwarz), exact
            const double radd = (double)(unsigned long long)(rad >> 64) * 18446744073709551616.0 + (double)(unsigned long long)rad;
            const float sigma = (float)(sqrt(radd) / ((double)cn * (double)qs));
            thr = fmaxf(thr, -(ct.top_n_sigma * sigma));
        }
    }
    // cut rows: the key of rank m0 (XTC), the draw's upper bound, and its logit, which the draw's weights are taken relative to -- exp((l -
    // mw) / T), 1 at rank m0 -- so that the fixed point keeps its 40 bits below the heaviest candidate, not below a token that is gone
    uint64_t kmax = ~0ull;
    float mw = mx;

    // Weighted select over K among the tokens with K >= kmin.  use_w = false: masses e = exp(l - mx); the LAST rank whose mass before
    // it is <= P * sum (the nucleus boundary).  use_w = true: masses w = exp((l - mx) / T); the FIRST rank whose mass up to and
    // including it is >= u * sum (the draw).  Returns the token index.
    // FILT, boundary only: by_mass = false drops the mass target (no mass atomics, no expf); ktarget != SAMPLE_NO_COUNT adds the count
    // target, the LAST rank with at most ktarget tokens before it.  The earlier of the two ranks is returned.  FILT, draw: the candidates
    // also pass the min-p test
    // DK (TYP only): std::true_type walks the typical order -- key typical_key, digit typical_digit -- for the boundary; the draw walks
    // the sampler's order with "typical_key >= kmin" as its candidate predicate
    // (always inlined: the typical kernel has three call sites, and a call would put the captured row state into scratch)
    auto select = [&](auto DK, bool use_w, uint64_t kmin, bool by_mass, uint32_t ktarget) __attribute__((always_inline)) -> uint32_t {
        constexpr bool dkey = decltype(DK)::value;
        bool live_p = FILT ? by_mass : true;                        // the target is still inside the chosen bins
        bool live_k = FILT ? ktarget != SAMPLE_NO_COUNT : false;
        uint32_t cbase = 0;             // number of the candidates' predecessors
        uint32_t sel0 = 0;              // pass-0 bin
        uint64_t prefix = 0;            // K bits [lo, 52) of the candidates (passes >= 2)
        uint32_t lo = 52;
        unsigned long long base = 0;    // mass of the candidates' predecessors
        unsigned long long target = 0;
        for (int p = 0; p < 6; ++p) {
            const uint32_t width = p == 5 ? 8 : 11, shift = p == 5 ? 0 : 52 - 11 * p;    // passes >= 1: K bits [shift, shift + width)
            for (uint32_t b = tid; b < SAMPLE_BINS; b += SAMPLE_THREADS) { sm.mass[b] = 0; sm.cnt[b] = 0; sm.idx[b] = 0; }
            if (tid == 0) {
                sm.sel = use_w ? 0u : 0xffffffffu;
                if constexpr (FILT) sm.selk = 0xffffffffu;
            }
            if constexpr (NPT > 0) {
                // keys are cheap to recompute; hoisted out of the pass loop they would take three more registers per element and spill
#pragma unroll
                for (int j = 0; j < NPT; ++j) asm volatile("" : "+v"(lv[j]));
            }
            __syncthreads();
            for_each([&](int j, float l) {
                const uint32_t i = tid + SAMPLE_THREADS * (uint32_t)j;
                uint64_t k;
                uint32_t c;
                bool cand;
                if constexpr (dkey) {
                    const float d = typical_dist(l, mx, gbar);
                    k = typical_key(d, i);
                    c = typical_digit(d, dscale);
                    cand = i < V;
                } else {
                    k = rank_key(l, i);
                    c = coarse_digit(l, mx, scale);
                    cand = i < V && k >= kmin;
                    if constexpr (TYP) {
                        if (typ) cand = i < V && typical_key(typical_dist(l, mx, gbar), i) >= kmin;
                    }
                }
                if constexpr (CUT) {
                    if (use_w) cand = cand && k <= kmax && (i == top || (l == mx ? 0.0f : l - mx) >= thr);   // thr > 0: p_max is below epsilon / eta, rank 0 alone
                } else if constexpr (FILT) {
                    if (use_w) cand = cand && (l == mx || l - mx >= ln_min_p);      // rank 0 always passes (mx = +inf: inf - inf is NaN)
                }
                if constexpr (MIRO) {
                    // rank 0 always passes; l == mx: surprise log2 W, as the mass pass weighs it (mx = +inf: inf - inf, 1 / T = inf: 0 * inf)
                    if (miro) cand = cand && (i == top || log2_w - (l == mx ? 0.0f : (l - mx) * inv_t) * SAMPLE_LOG2E <= mu);
                }
                if (p >= 1) cand = cand && c == sel0;
                if (p >= 2) cand = cand && (k >> lo) == prefix;
                if (cand) {
                    const uint32_t d = p == 0 ? c : (uint32_t)(k >> shift) & ((1u << width) - 1u);
                    if (live_p) {
                        float e;
                        if constexpr (CUT) e = use_w ? (l == mw ? 1.0f : expf((l - mw) * inv_t)) : (l == mx ? 1.0f : expf(l - mx));
                        else e = l == mx ? 1.0f : expf(use_w ? (l - mx) * inv_t : l - mx);
                        atomicAdd(&sm.mass[d], (unsigned long long)(e * SAMPLE_ONE));
                    }
                    atomicAdd(&sm.cnt[d], 1u);
                    atomicMax(&sm.idx[d], i);
                }
            });
            __syncthreads();
            // thread t owns bins dh = 2047 - 2t and dl = dh - 1: the exclusive scan in thread order is the mass of the higher bins
            const uint32_t dh = SAMPLE_BINS - 1 - 2 * tid, dl = dh - 1;
            const unsigned long long mh = sm.mass[dh], ml = sm.mass[dl];
            unsigned long long total = 0;
            unsigned long long above_h;
            uint32_t cabove_h = 0;      // tokens of the higher bins
            if constexpr (FILT) above_h = block_excl_scan2(mh + ml, sm.cnt[dh] + sm.cnt[dl], sm, &total, &cabove_h);
            else above_h = block_excl_scan(mh + ml, sm, &total);
            const unsigned long long above_l = above_h + mh;
            if (p == 0) {
                if (!use_w) {
                    if (live_p) target = (unsigned long long)floor((double)(dkey ? typical_p : top_p) * (double)total);
                } else {          // ceil(u * W), u = U / 2^24, in 128-bit integer arithmetic
                    const unsigned long long U = sample_splitmix(pr.seed, *step_word - pr.step_base) >> 40;
                    const unsigned long long plo = U * total, phi = __umul64hi(U, total);
                    target = (phi << 40) | (plo >> 24);
                    if (plo & 0xFFFFFFull) ++target;
                    if constexpr (MIRO) draw_total = total;
                }
            }
            if (!use_w) {
                if (live_p) {
                    if (sm.cnt[dl] && base + above_l <= target) atomicMin(&sm.sel, dl);
                    else if (sm.cnt[dh] && base + above_h <= target) atomicMin(&sm.sel, dh);
                }
                if constexpr (FILT) {
                    if (live_k) {
                        const uint32_t ch = sm.cnt[dh], cl = sm.cnt[dl];
                        if (cl && cbase + cabove_h + ch <= ktarget) atomicMin(&sm.selk, dl);
                        else if (ch && cbase + cabove_h <= ktarget) atomicMin(&sm.selk, dh);
                    }
                }
            } else {
                if (sm.cnt[dh] && base + above_h + mh >= target) atomicMax(&sm.sel, dh + 1);
                else if (sm.cnt[dl] && base + above_l + ml >= target) atomicMax(&sm.sel, dl + 1);
            }
            __syncthreads();
            // FILT: the words every thread reads back are pinned to scalar registers (the count select's state would otherwise cost ~25 VGPRs)
            const uint32_t raw = FILT ? __builtin_amdgcn_readfirstlane(sm.sel) : sm.sel;
            bool none = use_w ? raw == 0 : raw == 0xffffffffu;
            uint32_t d = use_w ? raw - 1 : raw;
            if constexpr (FILT) {
                if (!use_w) {
                    // the count target always finds a bin: the first bin that holds a token has nothing before it
                    const uint32_t dk = live_k ? __builtin_amdgcn_readfirstlane(sm.selk) : 0xffffffffu;
                    if (!live_p) { none = dk == 0xffffffffu; d = dk; }
                    else if (!none && live_k) {
                        if (dk == 0xffffffffu || dk < d) live_k = false;        // the nucleus ends first: its bin, the count target is dropped
                        else if (dk > d) { d = dk; live_p = false; }            // the top-k cut ends first
                    }
                }
            }
            if (!none && (d == dh || d == dl)) {
                sm.sel_above = d == dh ? above_h : above_l;
                sm.sel_cnt = sm.cnt[d];
                sm.sel_idx = sm.idx[d];
                if constexpr (FILT) sm.sel_cabove = d == dh ? cabove_h : cabove_h + sm.cnt[dh];
            }
            __syncthreads();
            if (none) return top;       // nothing qualifies (cannot happen in integer arithmetic): rank 0, find_or_first
            base += sm.sel_above;
            if constexpr (FILT) cbase += __builtin_amdgcn_readfirstlane(sm.sel_cabove);
            const uint32_t n = sm.sel_cnt, ix = sm.sel_idx;
            __syncthreads();            // sel / sel_* are rewritten by the next pass
            if (n == 1 || p == 5) return ix;
            if (p == 0) sel0 = d;
            else { prefix = p == 1 ? d : (prefix << width) | d; lo = shift; }
        }
        return top;
    };

    uint64_t kmin = 0;              // P >= 1: every token is in the nucleus
    const bool cut_p = !(top_p >= 1.0f), cut_k = FILT && top_k != 0;
    if (cut_p || cut_k) {           // kmin = max(kmin_P, kmin_K) in one descent; with cut_k alone it is count-only
        const uint32_t r = select(std::false_type{}, false, 0, cut_p, cut_k ? top_k - 1u : SAMPLE_NO_COUNT);
        const float lr = row[r];       // r < V: a token index
        kmin = rank_key(row_norm(lr), r);
    }
    if constexpr (TYP) {
        if (typ) {                  // the boundary of the typical order; the draw's kmin is a d-key
            const uint32_t r = select(std::true_type{}, false, 0, true, SAMPLE_NO_COUNT);
            const float lr = row[r];
            kmin = typical_key(typical_dist(row_norm(lr), mx, gbar), r);
        }
    }
    if constexpr (CUT) {
        if (xtc) {      // m' = #{candidates with p >= xtc_threshold} and the smallest of their keys, the key of rank m' - 1
            unsigned long long cn = 0, kmn = ~0ull;
            for_each([&](int j, float l) {
                const uint32_t i = tid + SAMPLE_THREADS * (uint32_t)j;
                const uint64_t k = rank_key(l, i);
                const float d = l == mx ? 0.0f : l - mx;
                const bool in = i < V && k >= kmin && (i == top || d >= thr) && d >= thr_x;
                cn += in ? 1ull : 0ull;
                kmn = in && k < kmn ? k : kmn;
            });
            cn = block_sum(cn, sm);
            kmn = block_min(kmn, sm);
            if (cn >= 2) {
                kmax = kmn;
                const uint32_t b = (uint32_t)(kmn >> 20);       // rank_key's monotone(logit), inverted
                mw = __uint_as_float((b & 0x80000000u) ? (b ^ 0x80000000u) : ~b);
            }
        }
    }
    const uint32_t tok = select(std::false_type{}, true, kmin, true, SAMPLE_NO_COUNT);
    if (tid == 0) {
        out[blockIdx.x] = tok;
        if constexpr (MIRO) {
            // the drawn token's surprise among the candidates, its own term from its logit (a weight of 2^-30 keeps ten bits in fixed point)
            if (miro && row_counts(gate, blockIdx.x)) {
                const float ly = row_norm(row[tok]);
                const float x = ly == mx ? 0.0f : (ly - mx) * inv_t;
                const float s = (log2f((float)draw_total) - 40.0f) - x * SAMPLE_LOG2E;
                alt[blockIdx.x].mu = mu - eta * (s - tau);
            }
        }
    }
}

// MODE SAMPLE_FILT: a top-k and a min-p cut per row (filt[row]).  SAMPLE_MIRO: Mirostat v2 per row (alt[row]: tau, eta and the running
// mu, rewritten when the draw counts).  SAMPLE_TYP: the locally typical cut per row (alt[row].typical_p).  A row whose own cut is off
// draws SAMPLE_PLAIN's token, bit for bit.  The arguments every mode reads come first: they are the preloaded kernarg words
template <int NPT, int MODE>
__global__ void __launch_bounds__(SAMPLE_THREADS) sample_rows_kernel(const float* __restrict__ logits, uint32_t V, uint32_t stride,
                                                                     const SampleParam* __restrict__ par, const uint32_t* __restrict__ step_word,
                                                                     uint32_t* __restrict__ out, const SampleFilter* __restrict__ filt,
                                                                     SampleAlt* alt, const RowGate gate, const SampleCut* __restrict__ cut) {
    __shared__ SampleSmem sm;
    sample_rows_body<NPT, MODE>(sm, logits, V, stride, par, filt, alt, gate, step_word, out, cut);
}

// The largest register copy (tokens per thread) of a mode; longer rows are re-read from L2.  Next to the count select's state of
// SAMPLE_FILT a 16-per-thread copy spills (88 bytes of scratch per lane), and so it does next to the Mirostat / typical state (DESIGN.md
// §7i): those keep 8 per thread, and their rows of 8193..16384 tokens are re-read
constexpr int sample_npt_max(int mode) { return mode == SAMPLE_PLAIN ? 16 : 8; }

template <int MODE>
static void sample_rows_mode(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const SamplePick& p, const uint32_t* step,
                             uint32_t* out) {
    constexpr int TOP = sample_npt_max(MODE);
    if (v <= 1024) sample_rows_kernel<1, MODE><<<n, SAMPLE_THREADS, 0, s>>>(logits, v, stride, p.par, step, out, p.filt, p.alt, p.gate, p.cut);
    else if (v <= 4096) sample_rows_kernel<4, MODE><<<n, SAMPLE_THREADS, 0, s>>>(logits, v, stride, p.par, step, out, p.filt, p.alt, p.gate, p.cut);
    else if (v <= TOP * 1024) sample_rows_kernel<TOP, MODE><<<n, SAMPLE_THREADS, 0, s>>>(logits, v, stride, p.par, step, out, p.filt, p.alt, p.gate, p.cut);
    else sample_rows_kernel<0, MODE><<<n, SAMPLE_THREADS, 0, s>>>(logits, v, stride, p.par, step, out, p.filt, p.alt, p.gate, p.cut);
}

int sample_rows(hipStream_t s, const float* logits, uint32_t v, uint32_t stride, uint32_t n, const SamplePick& pick, const uint32_t* step,
                uint32_t* out) {
    if (n == 0) return 0;
    if (v == 0 || v > SAMPLE_MAX_VOCAB || stride < v) return -1;
    switch (pick.mode) {
        case SAMPLE_FILT: sample_rows_mode<SAMPLE_FILT>(s, logits, v, stride, n, pick, step, out); break;
        case SAMPLE_MIRO: sample_rows_mode<SAMPLE_MIRO>(s, logits, v, stride, n, pick, step, out); break;
        case SAMPLE_TYP: sample_rows_mode<SAMPLE_TYP>(s, logits, v, stride, n, pick, step, out); break;
        case SAMPLE_CUT: sample_rows_mode<SAMPLE_CUT>(s, logits, v, stride, n, pick, step, out); break;
        default: sample_rows_mode<SAMPLE_PLAIN>(s, logits, v, stride, n, pick, step, out); break;
    }
    return 0;
}

}  // namespace wrk

int32_t wrk_sample_pack(wrk_ctx* ctx, const float* temperature, const float* top_p, const uint32_t* seed, uint32_t n,
                        std::vector<wrk::SampleParam>& out) {
    WRK_ARG(ctx, temperature && top_p && seed, "temperature, top_p and seed arrays are required");
    out.resize(n);
    for (uint32_t b = 0; b < n; ++b) {
        const float t = temperature[b], p = top_p[b];
        // +inf: 1 / T = 0 would weigh a -inf logit inside the nucleus with exp(-inf * 0) = exp(NaN)
        WRK_ARG(ctx, finite_f32(t) && t >= 0.0f, "temperature[%u] = %g: must be finite and >= 0", b, (double)t);
        WRK_ARG(ctx, !(p != p) && p >= 0.0f, "top_p[%u] = %g: must be >= 0", b, (double)p);
        out[b] = wrk::SampleParam{t, p, seed[b], 0u};
    }
    return WRK_OK;
}

int32_t wrk_filter_pack(wrk_ctx* ctx, const uint32_t* top_k, const float* min_p, uint32_t n, std::vector<wrk::SampleFilter>& out) {
    out.assign(n, wrk::SampleFilter{0u, -INFINITY});
    for (uint32_t b = 0; b < n; ++b) {
        if (top_k) out[b].top_k = top_k[b];
        if (!min_p) continue;
        const float p = min_p[b];
        WRK_ARG(ctx, !(p != p) && p >= 0.0f && p <= 1.0f, "min_p[%u] = %g: must be in [0, 1]", b, (double)p);
        out[b].ln_min_p = (float)std::log((double)p);       // f64, rounded once; min_p = 0: -inf, every token passes
    }
    return WRK_OK;
}

int32_t wrk_cut_pack(wrk_ctx* ctx, const wrk_cut_args& a, uint32_t n, std::vector<wrk::SampleCut>& out) {
    WRK_ARG(ctx, (a.xtc_probability != nullptr) == (a.xtc_threshold != nullptr), "xtc_probability and xtc_threshold: both arrays, or neither");
    out.assign(n, wrk::SampleCut{0.0f, -INFINITY, -INFINITY, 0.0f, 0.0f});
    auto unit = [](float x) { return !(x != x) && x >= 0.0f && x <= 1.0f; };
    for (uint32_t b = 0; b < n; ++b) {
        wrk::SampleCut& c = out[b];
        if (a.top_n_sigma) {
            const float s = a.top_n_sigma[b];
            WRK_ARG(ctx, !(s != s) && s >= 0.0f, "top_n_sigma[%u] = %g: must be >= 0", b, (double)s);
            c.top_n_sigma = s < FLT_MAX ? s : FLT_MAX;      // +inf: the largest finite value (inf * sigma with sigma = 0 would be NaN)
        }
        // the logarithms in f64, rounded once; 0: -inf, the cut is off
        if (a.epsilon_cutoff) {
            WRK_ARG(ctx, unit(a.epsilon_cutoff[b]), "epsilon_cutoff[%u] = %g: must be in [0, 1]", b, (double)a.epsilon_cutoff[b]);
            c.ln_epsilon = (float)std::log((double)a.epsilon_cutoff[b]);
        }
        if (a.eta_cutoff) {
            WRK_ARG(ctx, unit(a.eta_cutoff[b]), "eta_cutoff[%u] = %g: must be in [0, 1]", b, (double)a.eta_cutoff[b]);
            c.ln_eta = (float)std::log((double)a.eta_cutoff[b]);
        }
        if (a.xtc_probability) {
            const float p = a.xtc_probability[b], t = a.xtc_threshold[b];
            WRK_ARG(ctx, unit(p), "xtc_probability[%u] = %g: must be in [0, 1]", b, (double)p);
            WRK_ARG(ctx, unit(t), "xtc_threshold[%u] = %g: must be in [0, 1]", b, (double)t);
            c.xtc_probability = t > 0.5f ? 0.0f : p;        // above one half at most one token qualifies: off
            c.ln_xtc_threshold = (float)std::log((double)t);
        }
    }
    return WRK_OK;
}

int32_t wrk_mirostat_pack(wrk_ctx* ctx, const float* tau, const float* eta, const float* mu, uint32_t n, std::vector<wrk::SampleAlt>& out) {
    WRK_ARG(ctx, tau, "mirostat_eta / mirostat_mu without mirostat_tau");
    out.assign(n, wrk::SampleAlt{0.0f, 0.0f, 0.0f, 1.0f});
    for (uint32_t b = 0; b < n; ++b) {
        const float t = tau[b], e = eta ? eta[b] : 0.0f;
        WRK_ARG(ctx, finite_f32(t) && t >= 0.0f, "mirostat_tau[%u] = %g: must be finite and >= 0", b, (double)t);
        WRK_ARG(ctx, finite_f32(e) && e >= 0.0f, "mirostat_eta[%u] = %g: must be finite and >= 0", b, (double)e);
        const float m = mu ? mu[b] : 2.0f * t;       // a fresh sequence
        WRK_ARG(ctx, finite_f32(m), "mirostat_mu[%u] = %g: must be finite", b, (double)m);
        out[b] = wrk::SampleAlt{t, e, m, 1.0f};
    }
    return WRK_OK;
}

int32_t wrk_typical_pack(wrk_ctx* ctx, const float* typical_p, uint32_t n, std::vector<wrk::SampleAlt>& out) {
    out.assign(n, wrk::SampleAlt{0.0f, 0.0f, 0.0f, 1.0f});
    for (uint32_t b = 0; b < n; ++b) {
        const float p = typical_p[b];
        WRK_ARG(ctx, !(p != p) && p >= 0.0f && p <= 1.0f, "typical_p[%u] = %g: must be in [0, 1]", b, (double)p);
        out[b].typical_p = p;
    }
    return WRK_OK;
}

// the row functions' sampler: the filtered kernel on (top_k, min_p), either of which may be NULL; the Mirostat kernel on (tau, eta,
// mu_inout); the typical kernel on typical_p
struct sample_logits_kind {
    enum { PLAIN, FILTERED, MIROSTAT, TYPICAL, CUT } k = PLAIN;
    wrk_cut_args cut;           // CUT: the filtered kernel's arrays and these
    const uint32_t* top_k = nullptr; const float* min_p = nullptr;
    const float *tau = nullptr, *eta = nullptr; float* mu_inout = nullptr;
    const float* typical_p = nullptr;
};

static int32_t sample_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const float* temperature,
                             const float* top_p, const sample_logits_kind& kind, const uint32_t* seed, uint32_t step,
                             uint32_t* out_tokens, const char* who) {
    if (!ctx || !logits || !out_tokens) return WRK_E_ARG;
    std::lock_guard<std::recursive_mutex> lk(ctx->mu);
    const bool cutk = kind.k == sample_logits_kind::CUT;
    const bool filtered = kind.k == sample_logits_kind::FILTERED || cutk, miro = kind.k == sample_logits_kind::MIROSTAT,
               typical = kind.k == sample_logits_kind::TYPICAL;
    const uint32_t* top_k = kind.top_k;
    const float* min_p = kind.min_p;
    std::vector<wrk::SampleParam> par;
    std::vector<wrk::SampleFilter> filt;
    std::vector<wrk::SampleAlt> alt;
    std::vector<wrk::SampleCut> cut;
    int32_t rc = wrk_sample_pack(ctx, temperature, top_p, seed, n, par);
    if (rc == WRK_OK && filtered) rc = wrk_filter_pack(ctx, top_k, min_p, n, filt);
    if (rc == WRK_OK && cutk) rc = wrk_cut_pack(ctx, kind.cut, n, cut);
    if (rc == WRK_OK && miro) rc = wrk_mirostat_pack(ctx, kind.tau, kind.eta, kind.mu_inout, n, alt);
    if (rc == WRK_OK && typical) {
        WRK_ARG(ctx, kind.typical_p, "typical_p array required");
        rc = wrk_typical_pack(ctx, kind.typical_p, n, alt);
    }
    if (rc != WRK_OK) return rc;
    if (n == 0) return WRK_OK;
    rc = wrk_rows_check(ctx, logits, V, stride, n, who, wrk::SAMPLE_MAX_VOCAB);
    if (rc != WRK_OK) return rc;
    WRK_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(wrk::SampleAlt) >= sizeof(wrk::SampleFilter), "the rows at o_rows are sized for the larger struct");
    wrk_dev_arena dev;
    const size_t o_par = dev.add((size_t)n * sizeof(wrk::SampleParam)), o_step = dev.add(4), o_out = dev.add((size_t)n * 4);
    const size_t o_rows = dev.add((size_t)n * sizeof(wrk::SampleAlt));
    const size_t o_cut = dev.add(cutk ? (size_t)n * sizeof(wrk::SampleCut) : 0);
    WRK_HIP(ctx, dev.alloc());
    wrk::SamplePick pick{wrk::SAMPLE_PLAIN, dev.at<wrk::SampleParam>(o_par), nullptr, nullptr, wrk::RowGate{}};
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_par), par.data(), (size_t)n * sizeof(wrk::SampleParam), hipMemcpyHostToDevice, ctx->stream));
    WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_step), &step, 4, hipMemcpyHostToDevice, ctx->stream));
    if (filtered) {
        pick.mode = wrk::SAMPLE_FILT;
        pick.filt = dev.at<wrk::SampleFilter>(o_rows);
        WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_rows), filt.data(), (size_t)n * sizeof(wrk::SampleFilter), hipMemcpyHostToDevice, ctx->stream));
        if (cutk) {
            pick.mode = wrk::SAMPLE_CUT;
            pick.cut = dev.at<wrk::SampleCut>(o_cut);
            WRK_HIP(ctx, hipMemcpyAsync(dev.at<char>(o_cut), cut.data(), (size_t)n * sizeof(wrk::SampleCut), hipMemcpyHostToDevice, ctx->stream));
        }
    } else if (miro || typical) {
        pick.mode = miro ? wrk::SAMPLE_MIRO : wrk::SAMPLE_TYP;
        pick.alt = dev.at<wrk::SampleAlt>(o_rows);
        WRK_HIP(ctx, hipMemcpyAsync(pick.alt, alt.data(), (size_t)n * sizeof(wrk::SampleAlt), hipMemcpyHostToDevice, ctx->stream));
    }
    wrk::sample_rows(ctx->stream, (const float*)logits->ptr, V, stride, n, pick, dev.at<uint32_t>(o_step), dev.at<uint32_t>(o_out));
    WRK_LAUNCH_CHECK(ctx);
    WRK_HIP(ctx, hipMemcpyAsync(out_tokens, dev.at<char>(o_out), (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (miro && kind.mu_inout) WRK_HIP(ctx, hipMemcpyAsync(alt.data(), pick.alt, (size_t)n * sizeof(wrk::SampleAlt), hipMemcpyDeviceToHost, ctx->stream));
    WRK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (miro && kind.mu_inout)
        for (uint32_t b = 0; b < n; ++b) kind.mu_inout[b] = alt[b].mu;
    return WRK_OK;
}

extern "C" int32_t wrk_sample_logits(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const float* temperature,
                                     const float* top_p, const uint32_t* seed, uint32_t step, uint32_t* out_tokens) {
    return sample_logits(ctx, logits, V, stride, n, temperature, top_p, sample_logits_kind{}, seed, step, out_tokens, "wrk_sample_logits");
}

// both filter arrays NULL: wrk_sample_logits' kernel
extern "C" int32_t wrk_sample_logits_filtered(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n,
                                              const float* temperature, const float* top_p, const uint32_t* top_k, const float* min_p,
                                              const uint32_t* seed, uint32_t step, uint32_t* out_tokens) {
    sample_logits_kind kind;
    if (top_k || min_p) kind.k = sample_logits_kind::FILTERED;
    kind.top_k = top_k; kind.min_p = min_p;
    return sample_logits(ctx, logits, V, stride, n, temperature, top_p, kind, seed, step, out_tokens, "wrk_sample_logits_filtered");
}

// every cut array NULL: wrk_sample_logits_filtered's kernel
extern "C" int32_t wrk_sample_logits_cut(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n, const float* temperature,
                                         const float* top_p, const uint32_t* top_k, const float* min_p, const float* top_n_sigma,
                                         const float* epsilon_cutoff, const float* eta_cutoff, const float* xtc_probability,
                                         const float* xtc_threshold, const uint32_t* seed, uint32_t step, uint32_t* out_tokens) {
    sample_logits_kind kind;
    kind.cut = wrk_cut_args{top_n_sigma, epsilon_cutoff, eta_cutoff, xtc_probability, xtc_threshold};
    if (kind.cut.any()) kind.k = sample_logits_kind::CUT;
    else if (top_k || min_p) kind.k = sample_logits_kind::FILTERED;
    kind.top_k = top_k; kind.min_p = min_p;
    return sample_logits(ctx, logits, V, stride, n, temperature, top_p, kind, seed, step, out_tokens, "wrk_sample_logits_cut");
}

extern "C" int32_t wrk_sample_logits_mirostat(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n,
                                              const float* temperature, const float* top_p, const float* tau, const float* eta,
                                              float* mu_inout, const uint32_t* seed, uint32_t step, uint32_t* out_tokens) {
    sample_logits_kind kind;
    kind.k = sample_logits_kind::MIROSTAT;
    kind.tau = tau; kind.eta = eta; kind.mu_inout = mu_inout;
    return sample_logits(ctx, logits, V, stride, n, temperature, top_p, kind, seed, step, out_tokens, "wrk_sample_logits_mirostat");
}

extern "C" int32_t wrk_sample_logits_typical(wrk_ctx* ctx, const wrk_buf* logits, uint32_t V, uint32_t stride, uint32_t n,
                                             const float* temperature, const float* top_p, const float* typical_p, const uint32_t* seed,
                                             uint32_t step, uint32_t* out_tokens) {
    sample_logits_kind kind;
    kind.k = sample_logits_kind::TYPICAL;
    kind.typical_p = typical_p;
    return sample_logits(ctx, logits, V, stride, n, temperature, top_p, kind, seed, step, out_tokens, "wrk_sample_logits_typical");
}
