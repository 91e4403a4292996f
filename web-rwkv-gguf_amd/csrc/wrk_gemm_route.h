// Which MFMA kernel a matmul launch runs on, and with what geometry: gemm_plan() is the ONLY place these rules live.  Host only and pure:
// no HIP call, no environment variable, no static state -- the launchers (wrk_gemm.hip matmul_mfma_multi, wrk_gemm3.hip gemm_tile3_launch)
// read the switches (gemm_switches()), call gemm_plan() and launch what the plan says; tests/test_gemm_route_host.py asserts plans on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wrk_matjob.h"

namespace wrk {

constexpr int GEMM_MAX_JOBS = 8;
// tile edges of the kernels the plan counts workgroups for (the kernels' own constants are asserted equal where they are defined)
constexpr uint32_t ROUTE_TILE_ROWS = 64, ROUTE_TILE_TOK = 64, ROUTE_T3_ROWS = 128, ROUTE_T3_TOK = 128;

// every value an environment variable sets, with the defaults of an empty environment
struct GemmSwitches {
    // fewest stacked tokens sent to the matrix cores (tiles are padded to 16 tokens; below this the matvec kernels run).  Measured (1.5B
    // decode): 2 sequences break even, 3: 1.33 vs 1.79 ms, 8: 2x in favour of MFMA
    uint32_t min_tokens = 2;    // WRK_GEMM_MIN (>= 2)
    int ks_mode = 1;            // WRK_GEMM_KS: 0 off | 1 the measured routing | 2 every eligible launch
    int ks_bps = 0;             // WRK_KS_BPS: blocks per K slice, 0 = chosen here
    bool tile = true;           // WRK_GEMM_TILE=0: no LDS-tiled kernel (first or second generation)
    bool tile2 = true;          // WRK_GEMM_TILE2=0
    bool tile2_f16 = true;      // WRK_GEMM_TILE2_F16=0
    bool tile3 = true;          // WRK_GEMM_TILE3=0
    bool t3_split = true;       // WRK_T3_SPLIT=0: tile3 never splits K over workgroups (A/B)
    bool pair = false;          // WRK_GEMM_PAIR=1 (an A/B that lost, kept for its test)
};

enum GemmRoute : int {
    GEMM_NONE = 0,      // not for the MFMA path (the caller's -2: it falls back to the matvec kernels)
    GEMM_KSLICED,       // gemm_ks_kernel<nt, bps>
    GEMM_TILE3,         // xsum_kernel + gemm_tile3_kernel (+ t3_reduce_kernel)
    GEMM_TILE2,         // gemm_tile2_kernel<4>
    GEMM_TILE1,         // gemm_tile_kernel
    GEMM_KSPLIT,        // gemm_kernel<NT, NW> or gemm_pair_kernel<4>
    GEMM_ROUTES
};

// All jobs multiply the same number of tokens.  Jobs of one route share ONE launch; route[q] / wg_begin[q] are per job, wgs[r] is the x
// extent of route r's grid.  The per-launch parts are indexed by a job's position IN ITS LAUNCH (job order is kept).
struct GemmPlan {
    uint32_t n = 0;                             // stacked tokens
    GemmRoute route[GEMM_MAX_JOBS] = {};
    uint32_t wg_begin[GEMM_MAX_JOBS] = {};      // first workgroup (in x) of the job within its launch
    uint32_t wgs[GEMM_ROUTES] = {};
    struct KSliced {
        int nt = 0, bps = 0;                    // token tiles of 16; 256-blocks per K slice
        uint32_t nslices[GEMM_MAX_JOBS] = {};   // K slices per row group
        uint32_t rg_begin[GEMM_MAX_JOBS] = {};  // first row group of the job in the counter / partial space
        size_t lds_bytes = 0;                   // dynamic LDS: the staged activation slice
    } ks;
    struct Tile3 {
        uint32_t ttiles = 0;                    // token tiles (grid y); row tiles are wgs[GEMM_TILE3]
        uint32_t bps = 0, kslices = 1;          // kslices == 1: no K split (bps unused); else grid z, and a reduce launch
        int sums_of[GEMM_MAX_JOBS] = {};        // the earlier job of the launch whose input sums this one reads; its own index: it has its own
        size_t sh_off[GEMM_MAX_JOBS] = {}, sl_off[GEMM_MAX_JOBS] = {}, ts_off[GEMM_MAX_JOBS] = {};      // bytes into the scratch
        size_t part_off[GEMM_MAX_JOBS] = {};    // bytes into the scratch (K split only)
    } t3;
    struct KSplit {
        int nt = 0, nw = 0;                     // gemm_kernel<NT, NW>: 16-token tiles per wave, waves that split K
        bool pair = false;                      // gemm_pair_kernel<4> instead: wg_begin counts 32-row pairs
    } split;
};

// token tok = t + b * shape[1] of a [C, T, B] view sits at base + tok * stride[0] when the view covers the whole T extent of
// its parent (or has a single batch)
inline bool dense_stack(const DTensor& d) { return d.shape[2] == 1 || (d.shape[1] == d.stride[1] && d.offset[1] == 0); }
inline size_t stack_base(const DTensor& d) { return ((size_t)d.offset[2] * d.stride[1] + d.offset[1]) * d.stride[0] + d.offset[0]; }
inline uintptr_t stack_addr(const DTensor& d) { return (uintptr_t)d.p + stack_base(d) * (d.dtype == WRK_F16 ? 2 : 4); }       // of token 0

// is the job for the MFMA path at all (n < min_tokens, ROUND_F16, non-f16 / unaligned input, K % 32, Int8 / NF4 shapes: no)
inline bool gemm_ok(const MatJob& j, uint32_t n, const GemmSwitches& sw) {
    if (j.in.shape[1] * j.in.shape[2] != n || n < sw.min_tokens) return false;
    if (!dense_stack(j.in) || !dense_stack(j.out) || (j.has_res && !dense_stack(j.res))) return false;
    if (j.m < 4 || (j.m & 3u) || (j.out.dtype != WRK_F16 && j.out.dtype != WRK_F32) || (j.has_res && j.res.dtype != WRK_F16 && j.res.dtype != WRK_F32)) return false;
    // four consecutive output rows are stored (and residual rows loaded) as one vector
    if (((stack_base(j.out) | j.out.stride[0]) & 3u) || (j.has_res && ((stack_base(j.res) | j.res.stride[0]) & 3u))) return false;
    if (j.k < 32) return false;
    if (j.flags & WRK_MATRIX_ROUND_F16) return false;       // parity mode: per-element f16 rounding lives in the matvec kernels
    if (j.in.dtype != WRK_F16 || (j.k & 31u)) return false;
    // rows of the input views must be 16-byte aligned for the B-fragment loads
    if ((j.in.stride[0] & 7u) || (j.in.offset[0] & 7u)) return false;
    switch (j.kind) {
        case WRK_MAT_F16: case WRK_MAT_Q8_0: case WRK_MAT_Q6_K: case WRK_MAT_Q4_K: case WRK_MAT_Q5_K: return true;
        case WRK_MAT_INT8: return (j.k & 127u) == 0;      // rows aligned to the 128-element blocks
        case WRK_MAT_NF4: return (j.k & 63u) == 0 && j.aux != nullptr;
        default: return false;
    }
}

// the K-sliced kernel for the whole launch (decode batches, 5 .. 32 stacked tokens), or false: the other kernels
inline bool gemm_plan_ksliced(const MatJob* jobs, int njobs, uint32_t n, const GemmSwitches& sw, GemmPlan& P) {
    // Measured (1.5B Q4_K_M decode, ms per step: K-split kernels | this kernel for ffn.value only | for every launch; profiles/r02_ks_modes.txt):
    //   5 seq 1.265 | 1.222 | 1.382    8: 1.319 | 1.251 | 1.391    16: 1.498 | 1.390 | 1.468    24: 1.962 | 1.899 | 1.877
    //   32: 2.158 | 2.044 | 1.967      48: 3.150 | 3.981 | 3.803   64: 3.474 | 4.295 | 4.011
    // -> up to 16 tokens only the launch with few row tiles and long rows (ffn.value: 2048 rows x K = 8192, 13.8 -> 8.7 us at 16 tokens),
    // 17 .. 32 tokens every eligible launch, beyond that none (a 64-token slice is 32 KB per 256-block: the ingest problem again).
    // Each phase of the kernel is one memory round trip of ~2 us under load (stage | weights | tile out + count | tiles in), which is why it
    // only wins where the K-split kernel needs four dependent block iterations.
    const int mode = sw.ks_mode;
    if (mode <= 0 || !jobs[0].ks_part || !jobs[0].ks_cnt || n > 32) return false;
    const int nt = n <= 16 ? 1 : 2;
    bool all_q8 = false, any_other = false;
    for (int q = 0; q < njobs; ++q) {
        if (jobs[q].kind == WRK_MAT_Q8_0) all_q8 = true;
        else if (jobs[q].kind != WRK_MAT_F16) any_other = true;
    }
    all_q8 = all_q8 && !any_other;
    if (mode == 1 && n <= 16) {
        uint32_t tiles16 = 0, kmax = 0;
        for (int q = 0; q < njobs; ++q) { tiles16 += (jobs[q].m + 15) / 16; kmax = jobs[q].k > kmax ? jobs[q].k : kmax; }
        // round 3 (tools/ks_v6_sweep.sh, three RWKV-6 layers with D = 4096, ms per step, K-split kernels | this kernel with 2 | 4 blocks per slice):
        //   Q5_K x 16 streams 0.508 | 0.515 | 0.570, x 8 0.429 | - | 0.538        -> the K4 kinds keep the rule above
        //   Q8_0 x 16 streams 0.808 | 0.542 | 0.631, x 8 0.725 | - | 0.605        -> Q8_0 launches always come here (the K-split kernel's Q8_0
        //   body loads four row scales per 32-block and lane; here a slice's scales are one 16-byte load per row), two blocks per slice
        if (!(all_q8 || (tiles16 < 256 && kmax >= 4096))) return false;
    }
    for (int q = 0; q < njobs; ++q) {
        const MatJob& j = jobs[q];
        if (j.kind != WRK_MAT_Q4_K && j.kind != WRK_MAT_Q5_K && j.kind != WRK_MAT_Q6_K && j.kind != WRK_MAT_Q8_0 && j.kind != WRK_MAT_F16) return false;
        if (j.kind == WRK_MAT_Q8_0 && (j.row_bytes & 15u)) return false;       // the block scales of a slice are loaded as 16-byte vectors
        if ((j.k & 255u) || j.k < 256) return false;
    }
    // blocks per slice: as many as still give every CU a workgroup (fewer slices = fewer partial tiles to add); the staged activation
    // slice (16 nt tokens x bps x 256) has to fit the default 64 KB of dynamic LDS
    const int force_bps = sw.ks_bps;
    int bps = 0;
    for (int cand = (all_q8 && !force_bps) ? 2 : 4; cand >= 1 && !bps; cand >>= 1) {
        if (nt * cand > 4) continue;
        if (force_bps && cand != force_bps) continue;
        bool div = true;
        uint32_t wgs = 0;
        for (int q = 0; q < njobs; ++q) { const uint32_t nb = jobs[q].k >> 8; div = div && nb % cand == 0; wgs += ((jobs[q].m + 63) / 64) * (nb / cand); }
        if (div && (wgs >= 256 || cand == 1 || force_bps)) bps = cand;
    }
    if (!bps) return false;
    GemmPlan::KSliced ks;
    uint32_t wg_begin[GEMM_MAX_JOBS];
    uint32_t wg = 0, rg0 = 0;
    size_t floats = 0;
    for (int q = 0; q < njobs; ++q) {
        const uint32_t nsl = (jobs[q].k >> 8) / bps, nrg = (jobs[q].m + 63) / 64;
        if (nsl > 64) return false;
        wg_begin[q] = wg;
        ks.nslices[q] = nsl; ks.rg_begin[q] = rg0;
        wg += nrg * nsl; rg0 += nrg;
        floats += (size_t)nrg * nsl * 64 * 16 * nt;
    }
    // (row groups of one job are contiguous in the partial space: rg_begin counts row groups, the slices of a group sit side by side,
    // so the partial offset of job q is rg_begin x nslices_q tiles only when all jobs share nslices -- they do: one bps, and K differs
    // only between launches; checked here)
    for (int q = 1; q < njobs; ++q)
        if (ks.nslices[q] != ks.nslices[0]) return false;
    if (floats > jobs[0].ks_part_cap || rg0 > jobs[0].ks_cnt_cap) return false;
    ks.nt = nt; ks.bps = bps;
    ks.lds_bytes = (size_t)16 * nt * (bps * 256 + 8) * 2;       // f16
    P.ks = ks;
    for (int q = 0; q < njobs; ++q) { P.route[q] = GEMM_KSLICED; P.wg_begin[q] = wg_begin[q]; }
    P.wgs[GEMM_KSLICED] = wg;
    return true;
}

// The scratch layout and the K split of a tile3 launch over jobs cand[0 .. nc); false when the scratch (jobs[0].xsum, xsum_cap bytes)
// cannot hold the input sums
inline bool gemm_plan_tile3(const MatJob* jobs, const int* cand, int nc, uint32_t n, const GemmSwitches& sw, GemmPlan& P) {
    const size_t cap = jobs[0].xsum_cap;
    GemmPlan::Tile3 t3;
    uint32_t row_tiles = 0;
    // one pair of sum arrays per DISTINCT input (r, k, v of a layer read three different shifted inputs; a repeated one is summed once)
    size_t used = 0;
    for (int i = 0; i < nc; ++i) {
        const MatJob& j = jobs[cand[i]];
        row_tiles += (j.m + ROUTE_T3_ROWS - 1) / ROUTE_T3_ROWS;
        int hit = -1;
        for (int u = 0; u < i && hit < 0; ++u) {
            const MatJob& o = jobs[cand[u]];
            if (stack_addr(o.in) == stack_addr(j.in) && o.in.stride[0] == j.in.stride[0] && o.k == j.k) hit = u;
        }
        if (hit >= 0) { t3.sums_of[i] = t3.sums_of[hit]; t3.sh_off[i] = t3.sh_off[hit]; t3.sl_off[i] = t3.sl_off[hit]; t3.ts_off[i] = t3.ts_off[hit]; continue; }
        const size_t cnt = (size_t)n * (j.k >> 5), bytes = (cnt * 2 + 255) & ~(size_t)255, tbytes = ((size_t)n * 4 + 255) & ~(size_t)255;
        if (used + 2 * bytes + tbytes > cap) return false;
        t3.sums_of[i] = i; t3.sh_off[i] = used; t3.sl_off[i] = used + bytes; t3.ts_off[i] = used + 2 * bytes;
        used += 2 * bytes + tbytes;
    }
    // K split: one or two token tiles and fewer than ~160 workgroups -> slices of 4, 2 or 1 blocks (the first that fills the chip), all jobs of the
    // launch the same K.  Partial tiles behind the sum arrays in the launch's scratch; where they do not fit, the launch is not split.
    t3.ttiles = (n + ROUTE_T3_TOK - 1) / ROUTE_T3_TOK;
    bool same_k = true;
    for (int i = 1; i < nc; ++i) same_k = same_k && jobs[cand[i]].k == jobs[cand[0]].k;
    const uint32_t nb = jobs[cand[0]].k >> 8;
    if (same_k && t3.ttiles <= 2 && row_tiles * t3.ttiles < 160 && nb >= 2 && sw.t3_split) {
        uint32_t bps = 1;
        for (uint32_t c = 4; c >= 1; c >>= 1)
            if (nb % c == 0 && nb / c >= 2 && row_tiles * t3.ttiles * (nb / c) >= 160) { bps = c; break; }
        const uint32_t ks = (nb + bps - 1) / bps;
        const size_t at = (used + 255) & ~(size_t)255;
        size_t floats = 0;
        for (int i = 0; i < nc; ++i) { t3.part_off[i] = at + floats * 4; floats += (size_t)ks * n * jobs[cand[i]].m; }
        if (ks >= 2 && at + floats * 4 <= cap) { t3.bps = bps; t3.kslices = ks; }
    }
    P.t3 = t3;
    return true;
}

// The plan of one launch group; false (every route GEMM_NONE) when any job is not for the MFMA path.
inline bool gemm_plan(const MatJob* jobs, int njobs, const GemmSwitches& sw, GemmPlan& P) {
    P = GemmPlan();
    if (njobs <= 0 || njobs > GEMM_MAX_JOBS) return false;
    const uint32_t n = jobs[0].in.shape[1] * jobs[0].in.shape[2];
    P.n = n;
    for (int q = 0; q < njobs; ++q)
        if (!gemm_ok(jobs[q], n, sw)) return false;
    if (gemm_plan_ksliced(jobs, njobs, n, sw, P)) return true;

    // third-generation prefill tile (wrk_gemm3.hip): Q4_K / Q5_K, >= 128 stacked tokens, the launch's sum scratch at hand (round 3: from 128
    // tokens on, K split over workgroups for one or two token tiles).  A launch whose sums do not fit the scratch goes to the second-generation tile.
    int t3_jobs[GEMM_MAX_JOBS], nt3 = 0;
    if (sw.tile3 && jobs[0].xsum != nullptr && n >= 128)
        for (int q = 0; q < njobs; ++q) {
            const MatJob& j = jobs[q];
            // below 512 tokens the tile runs K-split (wrk_gemm3.hip) and pays a sum pre-pass and a reduce launch: measured (1.5B, tokens/s, this tile |
            // the kernels below): 128 tokens 21.5 k | 21.6 k with every matrix on it -- only the long rows gain (ffn value, K = 8192: 49.5 us -> 16 + 6.5 + 5);
            // 256 tokens 38.9 k | 35.8 k; 384 tokens (three token tiles, no split) 37.8 k | 46.6 k
            const bool t3_n = n >= 512 || (n > 128 && n <= 256) || (n == 128 && j.k >= 4096);
            if (t3_n && (j.kind == WRK_MAT_Q4_K || j.kind == WRK_MAT_Q5_K) && j.m >= 128 && j.in.shape[2] == 1 && (j.k & 255u) == 0) t3_jobs[nt3++] = q;
        }
    const GemmRoute t3_route = nt3 && gemm_plan_tile3(jobs, t3_jobs, nt3, n, sw, P) ? GEMM_TILE3 : GEMM_TILE2;
    for (int i = 0; i < nt3; ++i) P.route[t3_jobs[i]] = t3_route;

    // prefill regime: Q4_K / Q5_K / Q6_K / F16 matrices with >= 64 rows go to an LDS-tiled kernel, the rest (Int8, NF4, short) to the
    // K-split kernel, each group in one launch
    uint32_t kmax = 0;
    for (int q = 0; q < njobs; ++q) {
        const MatJob& j = jobs[q];
        if (P.route[q] == GEMM_NONE) {
            // the tile kernel walks the whole K in every wave: it needs enough workgroups to fill the chip (a 2048 x 8192
            // matrix x 128 tokens has only 64 tiles and is faster on the K-split kernel: 44 vs 74 us)
            const uint32_t tiles = ((j.m + ROUTE_TILE_ROWS - 1) / ROUTE_TILE_ROWS) * ((n + ROUTE_TILE_TOK - 1) / ROUTE_TILE_TOK);
            // (Q8_0 has a body in the second-generation tile kernel only: K % 128 == 0, rows in fours)
            // (round 3: from 48 tokens on -- the first-generation tile has no Q8_0 body, and the K-split kernel re-reads the activations per 16 rows)
            const bool q8_tile2 = j.kind == WRK_MAT_Q8_0 && sw.tile2 && n >= 48 && (j.k & 127u) == 0 && (j.m & 3u) == 0;
            const bool tile = sw.tile && n >= 48 && (j.kind == WRK_MAT_Q4_K || j.kind == WRK_MAT_Q5_K || j.kind == WRK_MAT_Q6_K || j.kind == WRK_MAT_F16 || q8_tile2) && j.m >= 64 &&
                              j.in.shape[2] == 1 && (tiles >= 96 || (j.k <= 2560 && tiles >= 64) ||    // enough workgroups, or a short serial walk,
                                                     (j.kind == WRK_MAT_F16 && j.k <= 2560));          // or a LoRA down-projection (64..320 rows): a handful of
            // tiles that ride along with the big matrices of their stage; on the K-split kernel they were a 32-us launch of 64 workgroups per layer
            // K4 kinds whose output rows come in fours (one vector store per lane) take the second-generation tile kernel
            // (with few workgroups -- a single 128-token chunk -- the first-generation kernel's longer stages are 4 % faster)
            const bool f16_tile2 = sw.tile2_f16 && j.kind == WRK_MAT_F16 && (j.k & 127u) == 0 && (j.row_bytes & 15u) == 0;
            if (tile && sw.tile2 && (n >= 512 || q8_tile2) && (j.kind == WRK_MAT_Q4_K || j.kind == WRK_MAT_Q5_K || q8_tile2 || f16_tile2) && (j.m & 3u) == 0) P.route[q] = GEMM_TILE2;
            else P.route[q] = tile ? GEMM_TILE1 : GEMM_KSPLIT;
        }
        const GemmRoute r = P.route[q];
        P.wg_begin[q] = P.wgs[r];
        if (r == GEMM_TILE3) P.wgs[r] += (j.m + ROUTE_T3_ROWS - 1) / ROUTE_T3_ROWS;
        else if (r == GEMM_KSPLIT) { P.wgs[r] += (j.m + 15) / 16; kmax = j.k > kmax ? j.k : kmax; }
        else P.wgs[r] += (j.m + ROUTE_TILE_ROWS - 1) / ROUTE_TILE_ROWS;
    }
    if (P.wgs[GEMM_KSPLIT]) {
        // tokens per wave: enough tiles to amortise the decode, few enough to keep >= ~2 waves per SIMD;
        // few row tiles x long rows (decode batches through ffn.value): 8 waves split K so a wave's serial chain is short
        // (measured, round 1: 16 waves x 2 blocks for K = 8192 is SLOWER, 23 vs 12 us at 2..16 tokens: 128 VGPRs per lane at 1024
        // threads spill the all-kinds kernel to scratch)
        const bool deep = P.wgs[GEMM_KSPLIT] < 256 && kmax >= 4096;
        P.split.nt = n > 64 ? 4 : n > 16 ? 2 : 1;
        P.split.nw = n <= 64 && deep ? 8 : 4;
        // two row tiles per workgroup where that still leaves >= ~200 workgroups (r, k, v + LoRA, ffn key at 16 tokens).  MEASURED SLOWER
        // (round 3, 1.5B decode, ms per step, pairs | single tiles: 8 sequences 1.339 | 1.244, 16 sequences 1.456 | 1.377): halving the
        // activation re-reads does not pay for twice the serial blocks per wave -- these launches are bound by the dependent chain of a
        // workgroup, not by the L2 bandwidth of the shared stack.  Off unless the switch is set (kept for the A/B and its test).
        bool pair = sw.pair && n <= 16 && !deep && P.wgs[GEMM_KSPLIT] >= 400;
        for (int q = 0; q < njobs; ++q)
            if (P.route[q] == GEMM_KSPLIT) pair = pair && (jobs[q].kind == WRK_MAT_Q4_K || jobs[q].kind == WRK_MAT_Q5_K || jobs[q].kind == WRK_MAT_F16);
        if (pair) {
            uint32_t wg2 = 0;
            for (int q = 0; q < njobs; ++q)
                if (P.route[q] == GEMM_KSPLIT) { P.wg_begin[q] = wg2; wg2 += (jobs[q].m + 31) / 32; }
            P.wgs[GEMM_KSPLIT] = wg2;
            P.split.pair = true;
        }
    }
    return true;
}

}  // namespace wrk
