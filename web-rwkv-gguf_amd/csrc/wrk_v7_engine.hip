// Persistent batch-1 decode engine for RWKV-7 on gfx950: ALL layers of one decode token in ONE launch, one workgroup per CU.
//
// Why: at batch 1 a layer is five dependent all-to-all steps; as five launches each of them costs a
// kernel boundary (~1.7 us) plus the next kernel's cold start (job struct, input vector, and only THEN the weight stream): 25 us for
// 38 MB, 18.7 % of the HBM roofline.  tools/probe/allgather_probe.hip measured the alternative on this chip: an in-launch all-to-all of a
// 4 KB vector through data-tagged granules (8-byte {payload, tag} written by one `sc1` store, re-read with `sc1` loads until every tag
// matches; no fence, no counter) costs 1.9 us, and it costs the SAME with a weight stream in flight if -- and only if -- the waves that
// poll are not the waves that stream (vector memory returns in issue order per wave).
//
// Structure.  384 threads: waves 0-3 compute (the thread mapping of the five-launch kernels: results are bit-identical to mode 1 with
// WRK_SPLIT_HEAD=0), wave 4 gathers (sweeps the granules of the next stage's input into LDS), wave 5 loads (streams this CU's slice of
// every stage's weights into LDS with LDS-DMA, `global_load_lds_dwordx4 ... nt`, a whole layer ahead: 148 KB of weights per CU and layer
// against 160 KB of LDS -- the round trip to HBM is off every one of the 120 dependent stages of a token).  The reference's analogue is
// the speculative job queue that hides the host's encode time behind the device (runtime/mod.rs:110-209); here it is the device's
// weight stream that runs ahead of the dependency chain.
//
// Stages of a layer (v7.rs:716-1007; the op list and rounding points of wrk_v7_fused.hip):
//   K1  LN1 + token shift -> r, k, v (quantised) + w1 (tanh) a1 g1 (sigmoid) v1          all workgroups, rows split by bytes
//   K2  LoRA up-projections, decay, kk, control_k, value lerp, WKV7, group norm, bonus, gate   one workgroup per head
//   K3  x += W_o . o                                                                      all workgroups
//   K5  LN2 + token shift -> relu(ffn key)^2                                              all workgroups
//   K6  x += ffn value . k ; ffn shift state ; (x *= 0.5 every `rescale` layers)           all workgroups, K over the 4 waves
// Hand-offs: K1 -> K2 (LoRA intermediates to every head, r / k / v to their head), K2 -> K3, K3 -> K5, K5 -> K6, K6 -> next K1.
//
// Safety: every spin is bounded; a give-up raises a device flag, the workgroup leaves at its next barrier, its consumers give up in
// turn, and the host reports WRK_E_HIP at the next synchronisation.  The grid is one workgroup per CU and needs all of them resident
// (LDS > 80 KB: exactly one per CU): the host refuses to build the engine otherwise.
#include "wrk_device.h"
#include "wrk_v7.h"
#include "wrk_dmv_body.h"
#include "wrk_v7_engine.h"
#include "wrk_lora_dev.h"

#include <algorithm>
#include <string>

namespace wrk {

#define ENG_LDS __attribute__((address_space(3)))
typedef ENG_LDS unsigned char lds_u8;

// workgroup barrier for all three roles: LDS traffic of this wave has landed, then s_barrier.  (Not __syncthreads(): its fences make the
// compiler drain vmcnt for pending LDS-DMA, and the roles must execute the same NUMBER of barrier instructions, nothing more.)
#define ENG_BAR() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

constexpr uint32_t ENG_SPIN_MAX = 1u << 21;

__device__ __forceinline__ uint32_t eng_tag(uint32_t layer, uint32_t stage) { return layer * 8u + stage + 1u; }

__device__ __forceinline__ void eng_store_granule(unsigned long long* g, uint32_t tag, uint32_t payload) {
    __hip_atomic_store(g, ((unsigned long long)tag << 32) | payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // global_store_dwordx2 sc1
}
__device__ __forceinline__ uint32_t pack_h2(float a, float b) {
    const f16x2 h = {(f16)a, (f16)b};
    return __builtin_bit_cast(uint32_t, h);
}

// ------------------------------------------------------------------ gather wave
// Sweep `n16` 16-byte pieces (two granules each) at `g` until every tag equals `tag`; the two payload dwords of piece q go to dst[2q],
// dst[2q + 1].  Eight loads per lane and pass, consecutive lanes on consecutive pieces.  false: gave up.
__device__ __forceinline__ bool eng_gather(const unsigned long long* g, uint32_t n16, uint32_t tag, ENG_LDS uint32_t* dst, uint32_t lane) {
    for (uint32_t base = 0; base < n16; base += 512) {
        const u32x4* p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = (const u32x4*)g + min(base + lane + 64u * i, n16 - 1);
        u32x4 v[8];
        bool good = false;
        for (uint32_t spins = 0; spins < ENG_SPIN_MAX; ++spins) {
            asm volatile(
                "global_load_dwordx4 %0, %8, off sc1\n\tglobal_load_dwordx4 %1, %9, off sc1\n\tglobal_load_dwordx4 %2, %10, off sc1\n\t"
                "global_load_dwordx4 %3, %11, off sc1\n\tglobal_load_dwordx4 %4, %12, off sc1\n\tglobal_load_dwordx4 %5, %13, off sc1\n\t"
                "global_load_dwordx4 %6, %14, off sc1\n\tglobal_load_dwordx4 %7, %15, off sc1\n\ts_waitcnt vmcnt(0)"
                : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7])
                : "v"(p[0]), "v"(p[1]), "v"(p[2]), "v"(p[3]), "v"(p[4]), "v"(p[5]), "v"(p[6]), "v"(p[7])
                : "memory");
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 8; ++i) ok &= (v[i].y == tag) & (v[i].w == tag);
            if (__all(ok)) { good = true; break; }
            __builtin_amdgcn_s_sleep(1);
        }
        if (!good) return false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t q = base + lane + 64u * i;
            if (q < n16) { dst[2 * q] = v[i].x; dst[2 * q + 1] = v[i].z; }
        }
    }
    return true;
}

// plain copy of n16 16-byte pieces (the launch's input vector, written by an earlier kernel)
__device__ __forceinline__ void eng_copy_in(const void* src, uint32_t n16, ENG_LDS u32x4* dst, uint32_t lane) {
    for (uint32_t q = lane; q < n16; q += 64) dst[q] = ((const u32x4*)src)[q];
}

// The ffn vector of K6.  Lane L of K-quarter wave kq multiplies chunk c of every row, i.e. elements [lo, lo + 16) and [hi, hi + 16) of
// the vector = 2 x 4 pieces of granules.  A quarter has one wave per row group, and they multiply the same chunks: the wave of row
// group 0 polls the `lo` pieces (half 0), the wave of row group 1 the `hi` pieces (half 1), so a CU fetches every granule once per
// pass.  The 16 payload elements go to `xe` (LDS, the vector's own element order); every K6 wave reads its chunks back from there
// behind the stage's first barrier (lds_x).  false: gave up.
template <int KIND>
__device__ __forceinline__ bool eng_sweep_half(const unsigned long long* g, uint32_t c, uint32_t half, uint32_t tag, ENG_LDS f16* xe) {
    uint32_t lo, hi;
    chunk_xoff<KIND>(c, lo, hi);
    const uint32_t off = half ? hi : lo;
    const u32x4* p = (const u32x4*)g + (off >> 2);
    u32x4 v[4];
    for (uint32_t spins = 0; spins < ENG_SPIN_MAX; ++spins) {
        asm volatile(
            "global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %4, off offset:16 sc1\n\tglobal_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
            "global_load_dwordx4 %3, %4, off offset:48 sc1\n\ts_waitcnt vmcnt(0)"
            : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
            : "v"(p)
            : "memory");
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) ok &= (v[i].y == tag) & (v[i].w == tag);
        if (__all(ok)) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u32x4 q = {v[2 * h].x, v[2 * h].z, v[2 * h + 1].x, v[2 * h + 1].z};
                *(ENG_LDS u32x4*)(xe + off + 8 * h) = q;
            }
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

// ------------------------------------------------------------------ loader wave
// `bytes` of weights at `src` (16-byte aligned, a multiple of 16) -> LDS at byte offset lds_off, in 1 KiB pieces; lanes beyond the end
// re-read the last 16 bytes into the slot's padding.  Returns the number of pieces issued.
__device__ __forceinline__ uint32_t eng_fill(const uint8_t* src, uint32_t bytes, lds_u8* smem, uint32_t lds_off, uint32_t lane) {
    if (bytes == 0) return 0;
    const uint32_t np = (bytes + 1023u) >> 10;
    for (uint32_t p = 0; p < np; ++p) {
        const uint32_t off = min(p * 1024u + lane * 16u, bytes - 16u);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + off), (ENG_LDS void*)(smem + lds_off + p * 1024u), 16, 0, 2);
    }
    return np;
}
// wait until at most n vector-memory operations of this wave are outstanding (rounded down to a multiple of 8: an immediate operand)
__device__ __forceinline__ void eng_wait_vm(uint32_t n) {
    if (n >= 56) asm volatile("s_waitcnt vmcnt(56)" ::: "memory");
    else if (n >= 48) asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
    else if (n >= 40) asm volatile("s_waitcnt vmcnt(40)" ::: "memory");
    else if (n >= 32) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ------------------------------------------------------------------ compute waves: weights and inputs from LDS
template <int KIND>
__device__ __forceinline__ Raw lds_raw(const lds_u8* row, uint32_t k, uint32_t c) {
    Raw r;
    r.w = *(const ENG_LDS u32x4*)(row + c * 16u);
    r.a = (u32x4){0, 0, 0, 0};
    r.b = (u32x2){0, 0};
    const uint32_t nb = k >> 8, b = c >> 3;
    if (KIND == WRK_MAT_Q4_K) {
        r.a.x = *(const ENG_LDS uint32_t*)(row + (nb * 128u + b * 4u));
        r.a.y = *(const ENG_LDS uint32_t*)(row + (nb * 132u + b * 16u + ((c & 7u) >> 1) * 4u));
    }
    return r;
}

template <int KIND>
__device__ __forceinline__ XRegs lds_x(const ENG_LDS f16* x, uint32_t c) {
    XRegs r;
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    r.v[0] = r.v[1] = r.v[2] = r.v[3] = z;
    r.s[0] = r.s[1] = 0.0f;
    uint32_t lo, hi;
    chunk_xoff<KIND>(c, lo, hi);
    r.v[0] = *(const ENG_LDS f16x8*)(x + lo);
    if (KIND != WRK_MAT_F16) {
        r.v[1] = *(const ENG_LDS f16x8*)(x + lo + 8);
        r.v[2] = *(const ENG_LDS f16x8*)(x + hi);
        r.v[3] = *(const ENG_LDS f16x8*)(x + hi + 8);
    }
    return r;
}

// lora_dot (wrk_lora_dev.h) with the token's LoRA intermediate read from LDS chunk by chunk (same products, same order)
template <int MAXCH>
__device__ __forceinline__ float eng_lora_dot(const f16x8 (&w)[MAXCH], const ENG_LDS f16* aux, uint32_t rank, uint32_t part) {
    float acc = 0.0f;
#pragma unroll
    for (int n = 0; n < MAXCH; ++n) {
        const uint32_t c = part * 8 + 32 * n;
        if (c < rank) {
            const f16x8 x = *(const ENG_LDS f16x8*)(aux + c);
            acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(w[n], w[n], 0, 1), __builtin_shufflevector(x, x, 0, 1), acc, false);
            acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(w[n], w[n], 2, 3), __builtin_shufflevector(x, x, 2, 3), acc, false);
            acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(w[n], w[n], 4, 5), __builtin_shufflevector(x, x, 4, 5), acc, false);
            acc = __builtin_amdgcn_fdot2(__builtin_shufflevector(w[n], w[n], 6, 7), __builtin_shufflevector(x, x, 6, 7), acc, false);
        }
    }
    acc += dpp_f32<0xB1>(acc);
    acc += dpp_f32<0x4E>(acc);
    return acc;
}

// NP pieces of a LoRA-2 unit from the packed image (wrk_lora2_pack.h), lane's 16 bytes of piece n into w[n]; the registers without a piece
// are zeroed (eng_lora_dot never multiplies them)
template <int NP>
__device__ __forceinline__ void eng_l2_load(f16x8 (&w)[8], const uint8_t* up) {
#pragma unroll
    for (int n = 0; n < NP; ++n) w[n] = *(const f16x8*)(up + n * ENG_L2_PIECE_BYTES);
    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int n = NP; n < 8; ++n) w[n] = z;
}

// what the epilogue of a row does with its dot product
struct EngFin {
    uint32_t act;           // activation
    float scale;            // wrk_matrix::out_scale
    const ENG_LDS f16* res; // residual vector (indexed by row), or nullptr
    float post;             // multiplied in after the residual add (rescale), 1 otherwise
};
__device__ __forceinline__ float eng_finish(const EngFin& f, uint32_t row, float v) {
    float o = act_apply(f.act, v * f.scale);
    if (f.res) o = r16(o) + (float)f.res[row];
    return o;
}

// Rows [r_begin, r_end) of the slot (relative to the workgroup's first row `row0`), one wave per row, lane L owns chunks L, L + 64, ...
// of every row (KS == 1) -- dmv_body's arithmetic with LDS-resident weights.  The range is a whole number of row pairs (eng_wave_rows;
// the host keeps a workgroup's row count even).  Rows are taken RB at a time; with RB == 4 and one chunk per lane a last pair is a
// batch of TWO rows: the same loop body, whose dot products, reductions and finish of the missing pair are skipped by a wave-uniform
// branch (a row's dot product does not depend on the batch it sits in).  Lane 0 publishes rows (0, 1) of a batch as one granule,
// lane 1 rows (2, 3) of a batch of four.  `gidx(row)` = granule index of the pair that starts at `row`.
template <int KIND, bool R16, int XI, int RB, class GIDX>
__device__ __forceinline__ void eng_rows(const lds_u8* slot, uint32_t row_bytes, uint32_t K, const ENG_LDS f16* xs, uint32_t row0, uint32_t r_begin,
                                         uint32_t r_end, const EngFin& fin, ENG_LDS uint32_t* pub, unsigned long long* gran, uint32_t tag, GIDX gidx,
                                         uint32_t lane) {
    if (r_begin >= r_end) return;
    const uint32_t kpad = (K + 15u) & ~15u;
    const uint32_t nch = num_chunks<KIND>(K, kpad);
    XRegs x[1][XI];
#pragma unroll
    for (int ci = 0; ci < XI; ++ci) {
        const uint32_t c = lane + 64u * ci;
        x[0][ci] = lds_x<KIND>(xs, min(c, nch - 1));
        if (c >= nch) {
            const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            x[0][ci].v[0] = x[0][ci].v[1] = x[0][ci].v[2] = x[0][ci].v[3] = z;
        }
        x_sums<KIND>(x[0][ci]);
    }
    static_assert(RB == 2 || RB == 4, "rows per batch");
    // The form of this loop is pinned by the register budget (profiles/engine_sched_resource_usage.txt: every instantiation at the
    // parent's figures).  The LDS reads of a batch stay unconditional and clamped to the last row; only the arithmetic is switched.
    // With more than one chunk per lane (D > 2048, and the F16 rows) the switch itself costs 5 - 12 spilled registers, so those
    // instantiations keep the padded last batch: the pair is computed with its second row repeated, and only the pair is published.
    constexpr bool PAD = XI > 1;
    for (uint32_t ri = r_begin; ri < r_end; ri += RB) {
        const bool whole = PAD || RB == 2 || ri + RB <= r_end;      // wave-uniform: the batch computes all its RB rows
        Raw raw[RB][XI];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            const lds_u8* rowp = slot + (size_t)min(ri + rb, r_end - 1) * row_bytes;
#pragma unroll
            for (int ci = 0; ci < XI; ++ci) raw[rb][ci] = lds_raw<KIND>(rowp, K, min(lane + 64u * ci, nch - 1));
        }
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
            if (rb < 2 || whole) {
                float acc[1] = {0.0f};
#pragma unroll
                for (int ci = 0; ci < XI; ++ci) dot_raw_tokens<KIND, R16, 1, XI>(raw[rb][ci], min(lane + 64u * ci, nch - 1), x, ci, acc);
                v[rb] = wave_sum(acc[0]);
            }
        if (lane < RB / 2) {
            const uint32_t ra = ri + 2 * lane;              // first row of this lane's pair
            if (ra < r_end) {                               // (a batch of two of RB == 4: lane 0 only)
                const float o0 = eng_finish(fin, row0 + ra, lane ? v[2] : v[0]) * fin.post;
                const float o1 = eng_finish(fin, row0 + ra + 1, lane ? v[3] : v[1]) * fin.post;
                if (pub) pub[ra >> 1] = pack_h2(o0, o1);    // published by ONE wave, coalesced (eng_publish)
                else eng_store_granule(gran + gidx(row0 + ra), tag, pack_h2(o0, o1));
            }
        }
    }
}

// The row pairs of a workgroup leave as granules from ONE wave, consecutive lanes on consecutive pairs.  Measured per stage (it costs a
// barrier): the ffn vector's hand-off (4 096 granules: 3.5 -> 2.6 us) gains from it; K1's and K3's do not (their 1.5 - 2.3 us turned out to
// be the loader's DMA bursts in front of the polls, not the scattered 8-byte stores) and keep storing from every wave.
template <class GIDX>
__device__ __forceinline__ void eng_publish(const ENG_LDS uint32_t* pub, uint32_t nrows, uint32_t row0, unsigned long long* gran, uint32_t tag, GIDX gidx,
                                            uint32_t lane) {
    for (uint32_t i = lane; 2 * i < nrows; i += 64) eng_store_granule(gran + gidx(row0 + 2 * i), tag, pub[i]);
}

// The statistics of an LN over x (LDS, f16 [K]), in the 256-thread mapping of the launches (same partial sums): the first four waves
// (`active`) keep their VPT vectors of 8 channels in xv, sum them shifted by c0 = x[0], and leave one partial sum per wave in red[0, 8).
// A barrier later eng_ln_stats gives every thread that asks the same mean and 1 / deviation.
template <int VPT>
__device__ __forceinline__ void eng_ln_partial(bool active, const ENG_LDS f16* xraw, ENG_LDS float* red, uint32_t K, f16x8 (&xv)[VPT], float& c0, uint32_t tid,
                                               uint32_t lane, uint32_t wave) {
    const uint32_t nvec = K >> 3;
    c0 = 0.0f;
    if (active) {
#pragma unroll
        for (int v = 0; v < VPT; ++v) xv[v] = *(const ENG_LDS f16x8*)(xraw + min(tid + 256u * v, nvec - 1) * 8);
        c0 = (float)xraw[0];
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int v = 0; v < VPT; ++v)
            if (tid + 256u * v < nvec)
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float dl = (float)xv[v][e] - c0; s1 += dl; s2 = __builtin_fmaf(dl, dl, s2); }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (lane == 0) { red[wave] = s1; red[4 + wave] = s2; }
    }
}
__device__ __forceinline__ void eng_ln_stats(const ENG_LDS float* red, float c0, uint32_t K, float eps, float& mean, float& dev) {
    const float a1 = (red[0] + red[1]) + (red[2] + red[3]);
    const float a2 = (red[4] + red[5]) + (red[6] + red[7]);
    const float md = a1 / (float)K;
    mean = c0 + md;
    dev = 1.0f / sqrtf(fmaxf(a2 / (float)K - md * md, 0.0f) + eps);
}

// LN + token shift of the layer input (dmv_body PRO 1, one input vector): x (LDS, f16) -> xs = mix(LN(x), prev, mixw), ln_out = LN(x).
// Two barriers inside.  The first four waves do the work; `active` = this wave is one of them.
template <int VPT>
__device__ __forceinline__ void eng_ln_mix(bool active, const ENG_LDS f16* xraw, ENG_LDS f16* xs, ENG_LDS f16* ln_out, ENG_LDS float* red, uint32_t K, float eps,
                                           const f16x8 (&wv)[VPT], const f16x8 (&bv)[VPT], const f16x8 (&mv)[VPT], const f32x4 (&pv)[VPT][2],
                                           uint32_t tid, uint32_t lane, uint32_t wave) {
    const uint32_t nvec = K >> 3;
    f16x8 xv[VPT];
    float c0;
    eng_ln_partial<VPT>(active, xraw, red, K, xv, c0, tid, lane, wave);
    ENG_BAR();
    if (active) {
        float mean, dev;
        eng_ln_stats(red, c0, K, eps, mean, dev);
#pragma unroll
        for (int v = 0; v < VPT; ++v) {
            const uint32_t i = tid + 256u * v;
            if (i >= nvec) continue;
            f16x8 yv, o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                yv[e] = (f16)__builtin_fmaf(((float)xv[v][e] - mean) * dev, (float)wv[v][e], (float)bv[v][e]);
                o[e] = (f16)wgsl_mix((float)yv[e], pv[v][e >> 2][e & 3], (float)mv[v][e]);
            }
            *(ENG_LDS f16x8*)(xs + i * 8) = o;
            *(ENG_LDS f16x8*)(ln_out + i * 8) = yv;
        }
    }
    ENG_BAR();
}

// ------------------------------------------------------------------ the kernel
// XD: 16-byte chunks per lane of a D-wide quantised row (D <= 2048 XD); R16: WRK_MATRIX_ROUND_F16; QK: kind of the big matrices;
// NCW: compute waves (8 or 14).  Wave NCW gathers, wave NCW + 1 loads.  A lone wave on a SIMD issues one vector instruction per ~4
// cycles, and the stages are instruction-issue bound (~125 instructions per row): the first build (4 compute waves, one per SIMD) spent
// 1.9 us on the 8 rows per wave of K1 -- hence as many compute waves as the register file allows.
// Barriers of a stage, the first one included.  EVERY role executes exactly these on every path: the compute waves in their stage
// bodies (each barrier there carries its number), the loader and the gather wave by replaying the counts (eng_replay).  The first
// ENG_K2_CHECKED barriers of K2, and the first barrier of every other stage, are the ones a give-up can be raised in front of: all
// three roles test the give-up flag behind each of them and leave the layer loop at the same barrier.  The flag is two words: between
// K2's (1) and (2) the gather wave is already sweeping again while a slow compute wave may not yet have read the flag behind (1), so a
// give-up of that second sweep is latched into abort_flag[1], which is read behind (2) only; abort_flag[0] is never written between a
// barrier and the reads behind it.
constexpr int ENG_LN_BARRIERS = 2;                          // eng_ln_mix: LN statistics | LN + shift written
constexpr int ENG_K1_BARRIERS = 2 + ENG_LN_BARRIERS;        // input in LDS | LN | K1 done
constexpr int ENG_K2_BARRIERS = 6;                          // (1) intermediates in | (2) r, k, v in + LoRA dots written | (3) | (4) | (5) | (6) K2 done
constexpr int ENG_K2_CHECKED = 2;                           // (1) and (2)
constexpr int ENG_K3_BARRIERS = 2;                          // input in LDS | K3 done
constexpr int ENG_K5_BARRIERS = 3 + ENG_LN_BARRIERS;        // input in LDS | LN | row pairs in `pub` | K5 done
constexpr int ENG_K6_BARRIERS = 3;                          // every wave has its inputs | partial sums written | K6 done
template <int N>
__device__ __forceinline__ void eng_replay() {
#pragma unroll
    for (int i = 0; i < N; ++i) ENG_BAR();
}
template <int XD, bool R16, int QK, int NCW>
__global__ void __launch_bounds__((NCW + 2) * 64) v7_engine_kernel(const EngArgs A, const uint32_t* __restrict__ wg_head) {
    extern __shared__ __attribute__((aligned(16))) unsigned char eng_smem_generic[];
    lds_u8* smem = (lds_u8*)eng_smem_generic;
    const EngShape& S = A.S;
    const uint32_t tid_all = threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid_all >> 6));
    const uint32_t wg = blockIdx.x;
    const uint32_t D = S.D, F = S.F;
    const uint32_t head = wg_head[2 * wg], k1r = wg_head[2 * wg + 1];       // head of this workgroup (or none); its rank among the K1 workgroups
    const bool is_head = head != ENG_NO_HEAD;
    ENG_LDS uint32_t* abort_flag = (ENG_LDS uint32_t*)(smem + S.lds_misc + 1008);       // [0]: every checked barrier but K2's (2); [1]: K2's (2)
    ENG_LDS float* red = (ENG_LDS float*)(smem + S.lds_misc);                // 8 floats
    ENG_LDS float* part = (ENG_LDS float*)(smem + S.lds_misc + 64);          // 32 rows x 4 K quarters
    ENG_LDS uint32_t* pub = (ENG_LDS uint32_t*)(smem + S.lds_misc + 64);     // K1 / K3 / K5: the payload of every row pair of the workgroup (<= 128)
    ENG_LDS f16* xraw0 = (ENG_LDS f16*)(smem + S.lds_xraw0);
    ENG_LDS f16* xraw1 = (ENG_LDS f16*)(smem + S.lds_xraw1);
    ENG_LDS f16* xs = (ENG_LDS f16*)(smem + S.lds_xs);
    ENG_LDS f16* lnbuf = (ENG_LDS f16*)(smem + S.lds_ln);
    // K2 scratch, behind xs
    ENG_LDS f16* auxbuf = (ENG_LDS f16*)(smem + S.lds_xs + D * 2u);          // aux_w | aux_a | aux_g | aux_v | r[64] k[64] v[64]
    const uint32_t naux = S.rw + S.ra + S.rg + S.rv;
    ENG_LDS float* k2f = (ENG_LDS float*)(smem + S.lds_xs + D * 2u + ((naux + 192u) * 2u + 15u & ~15u));      // ENG_K2F floats

    // this workgroup's share of every stage
    uint32_t j1 = ENG_K1_JOBS;
#pragma unroll
    for (int j = 0; j < ENG_K1_JOBS; ++j)
        if (k1r >= S.k1[j].wg0 && k1r < S.k1[j].wg0 + S.k1[j].nwg) j1 = j;
    const uint32_t k1_row0 = j1 < ENG_K1_JOBS ? (k1r - S.k1[j1].wg0) * S.k1[j1].rows_per_wg : 0u;
    const uint32_t k1_rows = j1 < ENG_K1_JOBS ? min(S.k1[j1].rows_per_wg, S.k1[j1].rows - k1_row0) : 0u;
    const uint32_t k1_rb = j1 < ENG_K1_JOBS ? S.k1[j1].row_bytes : 0u;
    const uint32_t k3_row0 = wg * S.k3_rpw, k3_rows = k3_row0 < D ? min(S.k3_rpw, D - k3_row0) : 0u;
    const uint32_t k5_row0 = wg * S.k5_rpw, k5_rows = k5_row0 < F ? min(S.k5_rpw, F - k5_row0) : 0u;
    const uint32_t k6_row0 = wg * S.k6_rpw, k6_rows = k6_row0 < D ? min(S.k6_rpw, D - k6_row0) : 0u;
    const uint32_t srows = S.state_rows;
    auto layer_state = [&](uint32_t l) { return A.state + ((size_t)l * A.num_batch + S.batch) * srows * D; };
    auto k1_src = [&](const EngLayer& L) -> const uint8_t* {
        const uint8_t* base = j1 == 0 ? L.w_r : j1 == 1 ? L.w_k : j1 == 2 ? L.w_v : j1 == 3 ? L.w1 : j1 == 4 ? L.a1 : j1 == 5 ? L.g1 : L.v1;
        return base + (size_t)k1_row0 * k1_rb;
    };
    auto k1_active = [&](uint32_t l) { return j1 < ENG_K1_JOBS && !(j1 == 6 && l == 0) && k1_rows > 0; };
    // timeline (WRK_TIMING=1): every wave stamps the 100 MHz clock into LDS (a global store here would put a ~1 us store into the wave's
    // vmcnt queue and distort what it measures); the stamps of the chosen layer are flushed when the layer is done
    ENG_LDS unsigned long long* lds_stamps = (ENG_LDS unsigned long long*)(smem + S.lds_misc + 1024);      // [NCW + 2][24]
#define ENG_STAMP(l, k)                                                                                                  \
    do {                                                                                                                 \
        if (A.stamps && (l) == A.stamp_layer && (tid_all & 63u) == 0) lds_stamps[wave * 24 + (k)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define ENG_STAMP0(l, k) ENG_STAMP(l, k)
#define ENG_FLUSH(l)                                                                                                     \
    do {                                                                                                                 \
        if (A.stamps && (l) == A.stamp_layer && (tid_all & 63u) < 24u)                                                   \
            A.stamps[((size_t)wg * (NCW + 2) + wave) * 24 + (tid_all & 63u)] = lds_stamps[wave * 24 + (tid_all & 63u)];   \
    } while (0)

    if (A.stamps && tid_all < (NCW + 2) * 24) lds_stamps[tid_all] = 0;
    if (tid_all == 0) { abort_flag[0] = 0; abort_flag[1] = 0; }
    ENG_BAR();

    // ================================================================== loader wave
    if (wave == NCW + 1) {
        const uint32_t lane = tid_all & 63u;
        uint32_t issued = 0, m1 = 0, m3 = 0, m5 = 0, m6 = 0;
        auto fill1 = [&](uint32_t l) { const EngLayer& L = A.layers[l]; issued += eng_fill(k1_src(L), k1_active(l) ? k1_rows * k1_rb : 0u, smem, S.lds_slot1, lane); m1 = issued; };
        auto fill3 = [&](uint32_t l) { const EngLayer& L = A.layers[l]; issued += eng_fill(L.w_o + (size_t)k3_row0 * S.rb_d, k3_rows * S.rb_d, smem, S.lds_slot3, lane); m3 = issued; };
        auto fill5 = [&](uint32_t l) { const EngLayer& L = A.layers[l]; issued += eng_fill(L.ffn_k + (size_t)k5_row0 * S.rb_d, k5_rows * S.rb_d, smem, S.lds_slot5, lane); m5 = issued; };
        auto fill6 = [&](uint32_t l) { const EngLayer& L = A.layers[l]; issued += eng_fill(L.ffn_v + (size_t)k6_row0 * S.rb_f, k6_rows * S.rb_f, smem, S.lds_slot6, lane); m6 = issued; };
        // WHEN a slot's DMA burst goes out matters: it sits in this CU's memory pipeline in front of the gather wave's polls.  Measured
        // schedules (1.5B, ms per token, launches 0.613): at the end of the slot's stage 0.628; one barrier later, i.e. when the next
        // stage's gather is over (this one) 0.604 - 0.608; every burst between the end of K1 and K3's gather 0.616 (the head workgroups'
        // K3 slot then lands late); a trickle of 6 / 10 pieces behind every barrier 0.79 / 0.73 (the loader arrives late at the LN
        // barriers).  profiles/r03_engine_ab.txt.
        // (kept: K1's slot is refilled the moment K1 ends -- nothing of this workgroup polls until K3's gather, 4 us later; the others go out
        // behind the first barrier of a stage whose own phase drains them before the NEXT gather polls: W_o's slot behind K5's, the ffn key
        // slot behind K6's, the ffn value slot behind the next K1's.  57 pieces behind K5's first barrier made the loader late at the LN
        // barriers (+1 us); the 47 KB K1 burst behind K3's ran into the x1 gather (2.3 us for that hand-off).)
        fill1(S.layer_begin); fill3(S.layer_begin); fill5(S.layer_begin); fill6(S.layer_begin);
        bool p6 = false;                                    // the previous layer's K6 has ended: its slot waits for this layer's K1
        for (uint32_t l = S.layer_begin; l < S.layer_end; ++l) {
            const bool more = l + 1 < S.layer_end;
            // K1
            eng_wait_vm(issued - m1);
            ENG_BAR();
            if (*abort_flag) break;
            if (p6) { fill6(l); p6 = false; }
            eng_replay<ENG_K1_BARRIERS - 1>();
            ENG_STAMP(l, 0);
            if (more) fill1(l + 1);                         // K1's own slot at once: until K3's gather this workgroup polls nothing (a head workgroup has no K1 rows)
            // K2
            if (is_head) {
                ENG_BAR();                                  // (1)
                if (*abort_flag) break;
                ENG_BAR();                                  // (2)
                if (abort_flag[1]) break;
                eng_replay<ENG_K2_BARRIERS - ENG_K2_CHECKED>();
            }
            // K3
            eng_wait_vm(issued - m3);
            ENG_BAR();
            if (*abort_flag) break;
            eng_replay<ENG_K3_BARRIERS - 1>();
            // K5
            eng_wait_vm(issued - m5);
            ENG_BAR();
            if (*abort_flag) break;
            if (more) fill3(l + 1);
            eng_replay<ENG_K5_BARRIERS - 1>();
            // K6
            eng_wait_vm(issued - m6);
            ENG_BAR();
            if (*abort_flag) break;
            if (more) fill5(l + 1);
            eng_replay<ENG_K6_BARRIERS - 1>();
            p6 = more;
            ENG_FLUSH(l);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return;
    }

    // ================================================================== gather wave
    if (wave == NCW) {
        const uint32_t lane = tid_all & 63u;
        for (uint32_t l = S.layer_begin; l < S.layer_end; ++l) {
            bool ok = true;
            // K1: the layer input
            if (l == S.layer_begin) eng_copy_in(A.x_row ? (const void*)((const f16*)A.x_in + (size_t)A.x_row[0] * D) : A.x_in, D >> 3, (ENG_LDS u32x4*)xraw0, lane);
            else ok = eng_gather(A.gran + S.g_x, D >> 2, eng_tag(l - 1, 4), (ENG_LDS uint32_t*)xraw0, lane);
            if (!ok && lane == 0) { *abort_flag = 1; atomicOr(A.fail, 1u); }
            ENG_STAMP(l, 0);
            ENG_BAR();
            if (*abort_flag) break;
            eng_replay<ENG_K1_BARRIERS - 1>();
            // K2: the LoRA intermediates, which the up-projections start on at once, then this head's r, k, v behind them in auxbuf
            if (is_head) {
                // (layer 0 has no value-residual LoRA: its granules are never written there)
                ok = eng_gather(A.gran + S.g_k1, (l == 0 ? naux - S.rv : naux) >> 2, eng_tag(l, 0), (ENG_LDS uint32_t*)auxbuf, lane);
                if (!ok && lane == 0) { *abort_flag = 1; atomicOr(A.fail, 2u); }
                ENG_STAMP(l, 4);
                ENG_BAR();                                  // (1)
                if (*abort_flag) break;
                ok = eng_gather(A.gran + S.g_k1 + S.g_aux + head * 96u, 48u, eng_tag(l, 0), (ENG_LDS uint32_t*)(auxbuf + naux), lane);
                if (!ok && lane == 0) { abort_flag[1] = 1; atomicOr(A.fail, 2u); }
                ENG_STAMP(l, 1);
                ENG_BAR();                                  // (2)
                if (abort_flag[1]) break;
                eng_replay<ENG_K2_BARRIERS - ENG_K2_CHECKED>();
            }
            // K3: the gated head outputs
            ok = eng_gather(A.gran + S.g_o, D >> 2, eng_tag(l, 1), (ENG_LDS uint32_t*)xs, lane);
            if (!ok && lane == 0) { *abort_flag = 1; atomicOr(A.fail, 4u); }
            ENG_STAMP(l, 2);
            ENG_BAR();
            if (*abort_flag) break;
            eng_replay<ENG_K3_BARRIERS - 1>();
            // K5: x after the time mix
            ok = eng_gather(A.gran + S.g_x1, D >> 2, eng_tag(l, 2), (ENG_LDS uint32_t*)xraw1, lane);
            if (!ok && lane == 0) { *abort_flag = 1; atomicOr(A.fail, 8u); }
            ENG_STAMP(l, 3);
            ENG_BAR();
            if (*abort_flag) break;
            eng_replay<ENG_K5_BARRIERS - 1>();
            // K6: the compute waves poll their own quarters of the ffn vector
            ENG_BAR();
            if (*abort_flag) break;
            eng_replay<ENG_K6_BARRIERS - 1>();
            ENG_FLUSH(l);
        }
        return;
    }

    // ================================================================== compute waves
    constexpr int VPT = XD;                                 // vectors of 8 channels per thread in the LN prologues
    constexpr int S64 = 64;
    constexpr int MAXU = (16 + NCW - 1) / NCW;              // (matrix, 16-row block) units of K2's LoRA up-projections per wave
    const uint32_t nvec = D >> 3;
    const float eps = S.ln_eps;
    const bool ln_wave = wave < 4;                          // the 256 threads of the launches' mapping
    const uint32_t c0 = is_head ? head * S64 : 0u;
    float vfirst_keep = 0.0f;                               // wave 0, lane = channel of the head
    if (is_head && S.layer_begin > 0 && wave == 0) vfirst_keep = (float)((const f16*)A.v_first)[c0 + (tid_all & 63u)];

    unsigned long long clk0 = 0, rt0 = 0;
    if (A.stamps && wg == 0 && tid_all == 0) { clk0 = __builtin_amdgcn_s_memtime(); rt0 = __builtin_amdgcn_s_memrealtime(); }
    for (uint32_t l = S.layer_begin; l < S.layer_end; ++l) {
        // Per-thread indices are re-derived every layer from an OPAQUE copy of the thread id: otherwise the compiler hoists every address
        // and offset that does not depend on the layer out of the loop and keeps ~100 registers of them alive through all stages.
        uint32_t tid = tid_all;
        asm volatile("" : "+v"(tid));
        const uint32_t lane = tid & 63u;
        float* lst = layer_state(l);
        const bool layer0 = l == 0;
        // everything of this layer that lives behind a pointer is fetched HERE, once, into registers (the barriers clobber memory: a
        // field read later would be a fresh dependent scalar round trip at the head of a stage)
        const f16* lv_base = (const f16*)A.vecs + (size_t)l * ENG_NV * D;
        auto lvec = [&](uint32_t idx) { return lv_base + (size_t)idx * D; };
        const float* scl = A.scal + (size_t)l * ENG_NS;
        const float sc_k1 = scl[j1 < ENG_K1_JOBS ? j1 : 0u], sc_o = scl[ENG_S_O], sc_fk = scl[ENG_S_FK], sc_fv = scl[ENG_S_FV];

        // ---- requests that depend on nothing: LN1 operands (the four LN waves).  A head workgroup has no K1 rows: it asks for the 64
        // channels of the LN it keeps instead (below)
        f16x8 wv[VPT], bv[VPT], mv[VPT];
        f32x4 pv[VPT][2];
        if (ln_wave && !is_head) {
            const f16* mixp = lvec(ENG_V_MIX0 + (j1 < ENG_K1_JOBS ? S.k1[j1].mix : 0u));
#pragma unroll
            for (int v = 0; v < VPT; ++v) {
                const uint32_t i = min(tid + 256u * v, nvec - 1);
                wv[v] = *(const f16x8*)(lvec(ENG_V_LN1W) + i * 8);
                bv[v] = *(const f16x8*)(lvec(ENG_V_LN1B) + i * 8);
                mv[v] = *(const f16x8*)(mixp + i * 8);
                pv[v][0] = *(const f32x4*)(lst + i * 8);
                pv[v][1] = *(const f32x4*)(lst + i * 8 + 4);
            }
        }

        // K5's LN operands are requested BEFORE K3 waits for its input, a stage and a hand-off before they are needed: requested at the end
        // of K3 they shared this CU's memory pipeline with the gather wave's polls for x1 (that hand-off took 2.0 us, its siblings 1.0)
        auto request_k5 = [&]() {
            if (ln_wave) {
                float* rowf = lst + (size_t)(srows - 1) * D;
    #pragma unroll
                for (int v = 0; v < VPT; ++v) {
                    const uint32_t i = min(tid + 256u * v, nvec - 1);
                    wv[v] = *(const f16x8*)(lvec(ENG_V_LN2W) + i * 8);
                    bv[v] = *(const f16x8*)(lvec(ENG_V_LN2B) + i * 8);
                    mv[v] = *(const f16x8*)(lvec(ENG_V_FFNXK) + i * 8);
                    pv[v][0] = *(const f32x4*)(rowf + i * 8);
                    pv[v][1] = *(const f32x4*)(rowf + i * 8 + 4);
                }
            }
        };
        if (!is_head) {
            // ================================================ K1
            ENG_BAR();                                      // x in xraw0, K1 weights in their slot
            if (*abort_flag) break;
            ENG_STAMP0(l, 1);
            eng_ln_mix<VPT>(ln_wave, xraw0, xs, lnbuf, red, D, eps, wv, bv, mv, pv, tid, lane, wave);
            ENG_STAMP0(l, 2);
            if (k1_active(l)) {
                const EngJob& J = S.k1[j1];
                uint32_t rb, re;
                eng_wave_rows(k1_rows, NCW, wave, rb, re);
                const EngFin fin{J.act, sc_k1, nullptr, 1.0f};
                const lds_u8* slot = smem + S.lds_slot1;
                ENG_LDS uint32_t* nopub = nullptr;
                if (J.f16) {
                    const uint32_t gb = S.g_k1 + J.gbase;
                    eng_rows<WRK_MAT_F16, false, 4 * XD, 2>(slot, k1_rb, D, xs, k1_row0, rb, re, fin, nopub, A.gran, eng_tag(l, 0),
                                                            [&](uint32_t r) { return gb + (r >> 1); }, lane);
                } else {
                    const uint32_t gb = S.g_k1 + S.g_aux + J.gbase * 32u;
                    eng_rows<QK, R16, XD, 4>(slot, k1_rb, D, xs, k1_row0, rb, re, fin, nopub, A.gran, eng_tag(l, 0),
                                             [&](uint32_t r) { return gb + (r >> 6) * 96u + ((r & 63u) >> 1); }, lane);
                }
            }
            ENG_STAMP0(l, 3);
            ENG_BAR();                                      // K1 done: slot, xs free
        } else {
            // ================================================ K1 on a head workgroup: no rows; the LoRA up-projection rows, per-channel
            // vectors and the state of K2 are requested NOW, a whole stage before they are needed (80 KB through one CU take 2 - 3 us).
            // Its LN1 is 64 channels wide, so it asks for no shift state, no mix vector and 64 elements of the LN weight and bias.
            // The compute waves stall ISSUING them: this workgroup passes the barrier below at ~2.6 us, with 64 coalesced loads as with the
            // 128 gathers before them (profiles/lora2_pack_ab.txt: one CU takes in 80 KB at ~32 GB/s).  Requested behind that barrier,
            // or with LN moved behind K2's barrier (1), the step was 3 % / 1 % slower (profiles/engine_sched_ab.txt).
            f16 h_lnw = 0, h_lnb = 0;                          // first in wave 1's queue: its LN waits for these two only
            if (wave == 1) { h_lnw = lvec(ENG_V_LN1W)[c0 + lane]; h_lnb = lvec(ENG_V_LN1B)[c0 + lane]; }
            // The LoRA rows come from the layer's packed image (wrk_lora2_pack.h): a unit is a run of 1 KB pieces in load order, and a
            // wave loads the pieces that exist (32 n < rank) -- 64 loads of consecutive bytes per workgroup at 1.5B, where the matrices
            // themselves took 128 loads of 64-byte pieces out of 16 rows each, half of them clamped re-reads that no dot used.  The same
            // 16 bytes reach the same lu[i][n] of the same lane.  A register without a piece is zero and never multiplied (eng_lora_dot);
            // layer 0's image has zeros for the value LoRA it does not have, and its dots are dropped below.  The image's address is
            // computed from a kernel argument, as the vectors' is: behind a pointer of EngLayer the loads were flat loads (they count
            // against lgkmcnt, so every ENG_BAR waited for them) behind a dependent fetch of the pointer.  One jump on the piece count
            // to a straight run of NP loads (profiles/lora2_pack_resource_usage.txt).
            const EngLora2Ranks R2{S.rw, S.ra, S.rg, S.rv};
            const uint8_t* l2_head = A.l2 + (l * eng_l2_layer_bytes(R2, S.H) + eng_l2_piece(R2, head, 0, 0) * ENG_L2_PIECE_BYTES);
            f16x8 lu[MAXU][8];
#pragma unroll
            for (int i = 0; i < MAXU; ++i) {
                const uint32_t u = wave + (uint32_t)i * NCW;                                          // a wave without a second unit loads nothing
                const uint32_t np = u < ENG_L2_UNITS ? eng_l2_pieces(eng_l2_rank(R2, u >> 2)) : 0u;
                const uint8_t* up = l2_head + (eng_l2_unit_piece(R2, u) * ENG_L2_PIECE_BYTES + lane * 16u);
                switch (np) {
                    case 1: eng_l2_load<1>(lu[i], up); break;
                    case 2: eng_l2_load<2>(lu[i], up); break;
                    case 3: eng_l2_load<3>(lu[i], up); break;
                    case 4: eng_l2_load<4>(lu[i], up); break;
                    case 5: eng_l2_load<5>(lu[i], up); break;
                    case 6: eng_l2_load<6>(lu[i], up); break;
                    case 7: eng_l2_load<7>(lu[i], up); break;
                    case 8: eng_l2_load<8>(lu[i], up); break;
                    default: eng_l2_load<0>(lu[i], up); break;
                }
            }
            float Sreg[16];
            const uint32_t ci64 = tid & 63u, g4 = tid >> 6;
            float* st = lst + (size_t)D + c0 + ci64;            // S[j][c0 + i] at st[j * D]
            if (ln_wave) {
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) Sreg[jj] = st[(size_t)(g4 * 16 + jj) * D];
            }
            f16 h_w0 = 0, h_a0 = 0, h_kk = 0, h_ka = 0, h_v0 = 0, h_gnw = 0, h_gnb = 0, h_rk = 0;
            if (wave == 0) {
                const uint32_t cc = c0 + lane;
                h_w0 = lvec(ENG_V_W0)[cc]; h_a0 = lvec(ENG_V_A0)[cc]; h_kk = lvec(ENG_V_KK)[cc]; h_ka = lvec(ENG_V_KA)[cc]; h_v0 = lvec(ENG_V_V0)[cc];
                h_gnw = lvec(ENG_V_GNW)[cc]; h_gnb = lvec(ENG_V_GNB)[cc]; h_rk = lvec(ENG_V_RK)[cc];
            }
            ENG_STAMP0(l, 19);
            ENG_BAR();                                      // x in xraw0
            if (*abort_flag) break;
            ENG_STAMP0(l, 1);
            // LN1 of a head workgroup: all that reads it is the att shift state of the head's own 64 channels (wave 1, behind barrier
            // (2)); nothing reads xs before K3's gather overwrites it.  So: eng_ln_mix's statistics, bit for bit (the same four waves,
            // elements and sums), then ONE wave normalises its 64 channels with eng_ln_mix's expression; no shift, no mix, and the same
            // ENG_LN_BARRIERS barriers, which the loader and the gather wave replay.
            {
                f16x8 xv[VPT];
                float x0;
                eng_ln_partial<VPT>(ln_wave, xraw0, red, D, xv, x0, tid, lane, wave);
                ENG_BAR();
                if (wave == 1) {
                    float mean, dev;
                    eng_ln_stats(red, x0, D, eps, mean, dev);
                    // The f32 result is made opaque before it is rounded to f16: for a lone `(f16)fmaf(..)` the compiler emits
                    // v_fma_mixlo_f16, which rounds the exact sum ONCE, where eng_ln_mix's eight-wide form is v_fma_f32 + v_cvt_f16_f32
                    // (rounded to f32, then to f16) -- one channel in a few thousand differed by an f16 ulp.
                    float y = __builtin_fmaf(((float)xraw0[c0 + lane] - mean) * dev, (float)h_lnw, (float)h_lnb);
                    asm volatile("" : "+v"(y));
                    lnbuf[c0 + lane] = (f16)y;
                }
                ENG_BAR();
            }
            ENG_STAMP0(l, 3);
            ENG_BAR();                                      // K1 done

            // ================================================ K2 (one workgroup per head): head_kernel's arithmetic
            ENG_LDS float* sh_r = k2f; ENG_LDS float* sh_w = k2f + 64; ENG_LDS float* sh_k = k2f + 128; ENG_LDS float* sh_v = k2f + 192;
            ENG_LDS float* sh_a = k2f + 256; ENG_LDS float* sh_b = k2f + 320; ENG_LDS float* sh_g = k2f + 384; ENG_LDS float* sh_kk = k2f + 448;
            ENG_LDS float* sh_red = k2f + 512;              // [4][64]: sa partials
            ENG_LDS float* sh_red2 = k2f + 768;             // [4][64]: y partials
            ENG_LDS float* sh_d = k2f + 1024;               // [4][64]: LoRA dots (w, a, g, v) per channel
            ENG_BAR();                                      // (1) LoRA intermediates in auxbuf[0, naux); r, k, v still on their way
            if (*abort_flag) break;
            ENG_STAMP0(l, 4);
            {
                const ENG_LDS f16* auxm[4] = {auxbuf, auxbuf + S.rw, auxbuf + S.rw + S.ra, layer0 ? auxbuf : auxbuf + S.rw + S.ra + S.rg};
#pragma unroll
                for (int i = 0; i < MAXU; ++i) {
                    const uint32_t u = wave + (uint32_t)i * NCW;
                    if (u < 16u) {
                        const uint32_t mi = u >> 2, bi = u & 3u;
                        const float dd = eng_lora_dot<8>(lu[i], auxm[mi], eng_l2_rank(R2, mi), lane & 3u);
                        if ((lane & 3u) == 0) sh_d[mi * 64 + 16 * bi + (lane >> 2)] = dd;
                    }
                }
            }
            ENG_STAMP0(l, 16);
            ENG_BAR();                                      // (2) r, k, v of this head behind them (the dots read below naux only); dots in sh_d
            if (abort_flag[1]) break;
            const ENG_LDS f16* hr = auxbuf + naux, *hk = hr + 64, *hv = hr + 128;
            if (wave == 0) {                                // per-channel stage: lane = channel of the head
                const float w0 = (float)h_w0, a0 = (float)h_a0, kkw = (float)h_kk, kaw = (float)h_ka;
                const float kraw = (float)hk[lane], rraw = (float)hr[lane];
                float v = (float)hv[lane];
                const float v0w = layer0 ? 0.0f : (float)h_v0, vfirst = layer0 ? 0.0f : vfirst_keep;
                const float dw = sh_d[lane], da = sh_d[64 + lane], dg = sh_d[128 + lane], dv = layer0 ? 0.0f : sh_d[192 + lane];
                const float w = r16(w0 + r16(dw));                                               // add(w0, w)
                const float a = r16(act_sigmoid(a0 + r16(da)));                                  // add_activate(.., Sigmoid)
                const float g = r16(dg);
                if (layer0) { vfirst_keep = v; ((f16*)A.v_first)[c0 + lane] = (f16)v; }          // blit(att_v, att_v0)
                else {
                    const float vv = r16(act_sigmoid(v0w + r16(dv)));
                    v = r16(wgsl_mix(v, vfirst, vv));                                            // lerp(att_v0, att_v, att_vv, reversed)
                }
                sh_w[lane] = __expf(-0.606531f * act_sigmoid(w));                                // act_w (time_mix_v7.wgsl:68-70)
                sh_g[lane] = g;
                sh_v[lane] = v;
                sh_r[lane] = rraw;
                const float kkv = r16(kkw * kraw);                                               // mul(k_k, kk)
                sh_k[lane] = r16(kraw * (1.0f + (a - 1.0f) * kaw));                              // control_k_v7
                // kk <- l2_norm(kk) over the head; a~ = -kk, b~ = kk * a
                const float nrm = 1.0f / sqrtf(wave_sum(kkv * kkv) + S.l2_eps);
                const float kkn = r16(kkv * nrm);
                sh_a[lane] = -kkn;
                sh_b[lane] = kkn * a;
                sh_kk[lane] = kkv;
            }
            if (wave == 1) lst[c0 + lane] = (float)lnbuf[c0 + lane];                             // att shift state <- LN1(x)
            ENG_STAMP0(l, 17);
            ENG_BAR();                                      // (3)
            if (ln_wave) {
                float sa = 0.0f;
                f32x4 av[4];                               // sh_a[16 g4 .. +15]: the same for every lane, four 16-byte reads
#pragma unroll
                for (int q = 0; q < 4; ++q) av[q] = *(const ENG_LDS f32x4*)(sh_a + g4 * 16 + 4 * q);
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) sa = __builtin_fmaf(Sreg[jj], av[jj >> 2][jj & 3], sa);
                sh_red[g4 * 64 + ci64] = sa;
            }
            ENG_BAR();                                      // (4)
            if (ln_wave) {
                const float sa = (sh_red[ci64] + sh_red[64 + ci64]) + (sh_red[128 + ci64] + sh_red[192 + ci64]);
                const float vv = sh_v[ci64];
                float y = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const f32x4 wq = *(const ENG_LDS f32x4*)(sh_w + g4 * 16 + 4 * q), kq4 = *(const ENG_LDS f32x4*)(sh_k + g4 * 16 + 4 * q);
                    const f32x4 bq = *(const ENG_LDS f32x4*)(sh_b + g4 * 16 + 4 * q), rq4 = *(const ENG_LDS f32x4*)(sh_r + g4 * 16 + 4 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int jj = 4 * q + e, j = g4 * 16 + jj;
                        const float sn = Sreg[jj] * wq[e] + kq4[e] * vv + sa * bq[e];
                        st[(size_t)j * D] = sn;
                        y = __builtin_fmaf(rq4[e], sn, y);
                    }
                }
                sh_red2[g4 * 64 + ci64] = y;
            }
            ENG_STAMP0(l, 18);
            ENG_BAR();                                      // (5)
            if (wave == 0) {
                float y = r16((sh_red2[lane] + sh_red2[64 + lane]) + (sh_red2[128 + lane] + sh_red2[192 + lane]));     // att_x <- y (f16 store)
                const float mean = wave_sum(y) * (1.0f / S64);
                const float dl = y - mean;
                const float var = wave_sum(dl * dl) * (1.0f / S64) + S.gn_eps;
                float o = r16(__builtin_fmaf(dl * (1.0f / sqrtf(var)), (float)h_gnw, (float)h_gnb));
                const float xx = wave_sum((float)h_rk * sh_k[lane] * sh_r[lane]);
                o = r16(o + xx * sh_v[lane]);
                o = sh_g[lane] * o;
                const float o_next = __shfl_down(o, 1, WAVE);
                if ((lane & 1u) == 0) eng_store_granule(A.gran + S.g_o + ((c0 + lane) >> 1), eng_tag(l, 1), pack_h2(o, o_next));
            }
            ENG_STAMP0(l, 5);
            ENG_BAR();                                      // (6) K2 done
        }

        // ================================================ K3: x1 = x + W_o . o
        request_k5();                                       // in flight across the K2 -> K3 hand-off
        ENG_BAR();                                          // o in xs, W_o rows in their slot
        if (*abort_flag) break;
        ENG_STAMP0(l, 6);
        {
            uint32_t rb, re;
            eng_wave_rows(k3_rows, NCW, wave, rb, re);
            const EngFin fin{WRK_ACT_NONE, sc_o, xraw0, 1.0f};
            const uint32_t gb = S.g_x1;
            ENG_LDS uint32_t* nopub = nullptr;
            eng_rows<QK, R16, XD, 2>(smem + S.lds_slot3, S.rb_d, D, xs, k3_row0, rb, re, fin, nopub, A.gran, eng_tag(l, 2),
                                     [&](uint32_t r) { return gb + (r >> 1); }, lane);
        }
        ENG_STAMP0(l, 7);
        ENG_BAR();                                          // K3 done

        // ================================================ K5: k = relu(ffn_key . mix(LN2(x1)))^2
        ENG_BAR();                                          // x1 in xraw1, ffn key rows in their slot
        if (*abort_flag) break;
        ENG_STAMP0(l, 8);
        eng_ln_mix<VPT>(ln_wave, xraw1, xs, lnbuf, red, D, eps, wv, bv, mv, pv, tid, lane, wave);
        ENG_STAMP0(l, 14);
        {
            uint32_t rb, re;
            eng_wave_rows(k5_rows, NCW, wave, rb, re);
            const EngFin fin{WRK_ACT_SQUARED_RELU, sc_fk, nullptr, 1.0f};
            const uint32_t gb = S.g_k;
            eng_rows<QK, R16, XD, 4>(smem + S.lds_slot5, S.rb_d, D, xs, k5_row0, rb, re, fin, pub, A.gran, eng_tag(l, 3), [&](uint32_t r) { return gb + (r >> 1); }, lane);
            ENG_BAR();
            if (wave == 0) eng_publish(pub, k5_rows, k5_row0, A.gran, eng_tag(l, 3), [&](uint32_t r) { return gb + (r >> 1); }, lane);
        }
        ENG_STAMP0(l, 9);
        ENG_BAR();                                          // K5 done

        // ================================================ K6: x = x1 + ffn_value . k   (K over four waves, rows over NCW / 4 groups)
        {
            // The two waves (kq, 0) and (kq, 1) of a K quarter poll one half each of the quarter's granules into the exchange area `xe`
            // (eng_sweep_half): a CU fetches the vector once per pass.  They poll whenever the workgroup has rows at all -- their own
            // row group may be empty, their partner's is not.  `xe` lies over xs and K2's scratch, which nothing reads between K5's
            // rows and the next layer's LN; the host has checked that it fits (wrk_v7_engine_create).
            constexpr uint32_t NG = NCW / 4;                // row groups
            const uint32_t kq = wave & 3u, grp = wave >> 2;
            const bool k6_wave = grp < NG;
            const uint32_t rq = (k6_rows + NG - 1) / NG;
            const uint32_t g_b = min(grp * rq, k6_rows), g_e = min(g_b + rq, k6_rows);
            const uint32_t kpad = (F + 15u) & ~15u;
            const uint32_t nch = num_chunks<QK>(F, kpad);
            const uint32_t cbase = lane + 64u * kq;
            ENG_LDS f16* xe = xs;
            bool swept = true;
            if (grp < 2 && k6_rows > 0) {
#pragma unroll
                for (int ci = 0; ci < XD; ++ci)
                    if (swept) swept = eng_sweep_half<QK>(A.gran + S.g_k, min(cbase + 256u * ci, nch - 1), grp, eng_tag(l, 3), xe);
            }
            if (!swept && lane == 0) { *abort_flag = 1; atomicOr(A.fail, 16u); }
            ENG_STAMP0(l, 10);
            ENG_BAR();                                      // ffn value rows in their slot (loader), the whole ffn vector in xe
            if (*abort_flag) break;                         // (xe is read behind this test only: a give-up feeds no row)
            ENG_STAMP0(l, 11);
            // The read-back is unconditional (a wave without rows reads and drops it): behind the branch "this wave has rows" it cost
            // 30 - 80 spilled registers in every instantiation (profiles/ffn_sweep_resource_usage.txt).
            XRegs x[1][XD];
#pragma unroll
            for (int ci = 0; ci < XD; ++ci) {
                const uint32_t c = cbase + 256u * ci;
                x[0][ci] = lds_x<QK>(xe, min(c, nch - 1));
                if (c >= nch) {
                    const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
                    x[0][ci].v[0] = x[0][ci].v[1] = x[0][ci].v[2] = x[0][ci].v[3] = z;
                }
                x_sums<QK>(x[0][ci]);
            }
            ENG_STAMP0(l, 15);
            const lds_u8* slot = smem + S.lds_slot6;
            if (k6_wave)
                for (uint32_t ri = g_b; ri < g_e; ri += 4) {
                    Raw raw[4][XD];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) {
                        const lds_u8* rowp = slot + (size_t)min(ri + rb, g_e - 1) * S.rb_f;
#pragma unroll
                        for (int ci = 0; ci < XD; ++ci) raw[rb][ci] = lds_raw<QK>(rowp, F, min(cbase + 256u * ci, nch - 1));
                    }
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) {
                        float acc[1] = {0.0f};
#pragma unroll
                        for (int ci = 0; ci < XD; ++ci) dot_raw_tokens<QK, R16, 1, XD>(raw[rb][ci], min(cbase + 256u * ci, nch - 1), x, ci, acc);
                        const float pvs = wave_sum(acc[0]);
                        if (lane == 0 && ri + rb < g_e) part[(ri + rb) * 4 + kq] = pvs;
                    }
                }
        }
        ENG_STAMP0(l, 12);
        ENG_BAR();
        if (wave == 0) {                                    // one wave finishes the (at most 32) rows
            const bool valid = lane < k6_rows;
            const uint32_t r = k6_row0 + min(lane, k6_rows ? k6_rows - 1 : 0u);
            float o = 0.0f;
            if (k6_rows) {
                const uint32_t p = min(lane, k6_rows - 1);
                o = ((part[p * 4] + part[p * 4 + 1]) + (part[p * 4 + 2] + part[p * 4 + 3])) * sc_fv;
                o = r16(o) + (float)xraw1[r];
                if ((l + 1) % S.rescale == 0) o = r16(o) * 0.5f;                              // affine(x, 0.5) after the layer
            }
            const float o_next = __shfl_down(o, 1, WAVE);
            if (valid) {
                lst[(size_t)(srows - 1) * D + r] = (float)lnbuf[r];                           // ffn shift state <- LN2(x1)
                if ((lane & 1u) == 0) eng_store_granule(A.gran + S.g_x + (r >> 1), eng_tag(l, 4), pack_h2(o, o_next));
                if (l + 1 == S.layer_end) ((f16*)A.x_out)[r] = (f16)o;
            }
        }
        ENG_STAMP0(l, 13);
        ENG_BAR();                                          // K6 done
        ENG_FLUSH(l);
    }
    if (A.stamps && wg == 0 && tid_all == 0) {              // shader clock over the launch: (cycles, 100 MHz ticks) behind the timeline
        unsigned long long* tail = A.stamps + (size_t)S.nwg * 16 * 24;
        tail[0] = __builtin_amdgcn_s_memtime() - clk0;
        tail[1] = __builtin_amdgcn_s_memrealtime() - rt0;
    }
#undef ENG_STAMP
#undef ENG_STAMP0
#undef ENG_FLUSH
}

}  // namespace wrk

// ------------------------------------------------------------------ host
struct wrk_v7_engine {
    wrk_v7_model* m = nullptr;
    wrk::EngShape S{};
    wrk::EngLayer* layers = nullptr;        // device [L]
    void* vecs = nullptr;                   // device f16 [L][ENG_NV][D]
    float* scal = nullptr;                  // device [L][ENG_NS]
    uint32_t* wg_head = nullptr;            // device [nwg]
    unsigned long long* gran = nullptr;     // device
    uint32_t* fail = nullptr;               // device (pinned readable through memcpy)
    unsigned long long* stamps = nullptr;   // device, WRK_TIMING=1
    uint8_t* l2pack = nullptr;              // device: the packed LoRA up-projections of every layer (wrk_lora2_pack.h)
    void* emb_ln = nullptr;                 // device f16 [V][D]: LN(ln0) of every embedding row (the same kernel as the step's embedding launch)
    bool r16 = false;
    int xd = 1, ncw = 8;
    uint32_t quant = 0;
};

static uint32_t up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

typedef void (*eng_fn)(const wrk::EngArgs, const uint32_t*);
static eng_fn eng_kernel(int xd, bool r16, int ncw) {
    using namespace wrk;
#define ENG_PICK(XD_, R_) (ncw == 14 ? (eng_fn)v7_engine_kernel<XD_, R_, WRK_MAT_Q4_K, 14> : (eng_fn)v7_engine_kernel<XD_, R_, WRK_MAT_Q4_K, 8>)
    if (xd == 1) return r16 ? ENG_PICK(1, true) : ENG_PICK(1, false);
    return r16 ? ENG_PICK(2, true) : ENG_PICK(2, false);
#undef ENG_PICK
}
static const void* eng_kernel_fn(int xd, bool r16, int ncw) { return (const void*)eng_kernel(xd, r16, ncw); }

int32_t wrk_v7_engine_create(wrk_v7_model* m, wrk_v7_engine** out) {
    using namespace wrk;
    wrk_ctx* ctx = m->ctx;
    *out = nullptr;
    const auto& d = m->d;
    const uint32_t D = d.num_emb, F = d.num_hidden, H = d.num_head, NWG = (uint32_t)ctx->num_cu;
    auto no = [&](const char* why) { return wrk_fail(ctx, WRK_E_UNSUPPORTED, "decode engine: %s", why); };
    if (m->act_dtype != WRK_F16) return no("f32 frames");
    if (H == 0 || D != H * 64 || D % 256 || D > 4096 || F % 1024 || F != 4 * D) return no("shape");
    if (d.lora_w % 8 || d.lora_a % 8 || d.lora_g % 8 || d.lora_v % 8 || d.lora_w < 8 || d.lora_a < 8 || d.lora_g < 8 || d.lora_v < 8 ||
        d.lora_w > 128 || d.lora_a > 128 || d.lora_v > 128 || d.lora_g > 256 || ((d.lora_w + d.lora_a + d.lora_g + d.lora_v) % 16))
        return no("LoRA ranks");
    if (NWG < 2 * H || NWG < 64) return no("too few compute units");
    // every big matrix of one quantised kind (Q4_K: the headline configuration), LoRA matrices F16, one rounding mode
    uint32_t quant = 0xffffffffu, flags = 0xffffffffu;
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const auto& L = m->layers[li];
        const wrk_matrix* big[] = {L.w_r, L.w_k, L.w_v, L.w_o, L.ffn_w_k, L.ffn_w_v};
        for (const wrk_matrix* q : big) {
            if (quant == 0xffffffffu) { quant = q->kind; flags = q->flags; }
            if (q->kind != quant || q->flags != flags) return no("mixed matrix kinds");
        }
        const wrk_matrix* lo[] = {L.w1, L.a1, L.g1, li ? L.v1 : L.a1, L.w2, L.a2, L.g2, li ? L.v2 : L.a2};
        for (const wrk_matrix* q : lo)
            if (!q || q->kind != WRK_MAT_F16) return no("LoRA matrices must be F16");
        if (L.w_r->k != D || L.w_r->m != D || L.ffn_w_k->m != F || L.ffn_w_v->k != F || L.w1->m != d.lora_w || L.a1->m != d.lora_a ||
            L.g1->m != d.lora_g || (li && L.v1->m != d.lora_v) || L.w2->k != d.lora_w || L.a2->k != d.lora_a || L.g2->k != d.lora_g ||
            (li && L.v2->k != d.lora_v) || L.w2->m != D || L.a2->m != D || L.g2->m != D || (li && L.v2->m != D))
            return no("matrix shapes");
    }
    if (quant != WRK_MAT_Q4_K) return no("only Q4_K matrices so far");
    if (m->layers.empty()) return no("no layers");

    wrk_v7_engine* e = new wrk_v7_engine();
    e->m = m;
    e->quant = quant;
    e->r16 = (flags & WRK_MATRIX_ROUND_F16) != 0;
    e->xd = D <= 2048 ? 1 : 2;
    EngShape& S = e->S;
    S.D = D; S.F = F; S.H = H; S.nwg = NWG;
    S.rw = d.lora_w; S.ra = d.lora_a; S.rg = d.lora_g; S.rv = d.lora_v;
    const auto& L0 = m->layers[0];
    S.rb_d = (uint32_t)L0.w_r->row_bytes; S.rb_f = (uint32_t)L0.ffn_w_v->row_bytes;
    for (const auto& L : m->layers) {
        if (L.w_r->row_bytes != S.rb_d || L.w_k->row_bytes != S.rb_d || L.w_v->row_bytes != S.rb_d || L.w_o->row_bytes != S.rb_d ||
            L.ffn_w_k->row_bytes != S.rb_d || L.ffn_w_v->row_bytes != S.rb_f) { delete e; return no("row strides differ between layers"); }
    }
    // ---- K1: workgroups to matrices in proportion to bytes; rows per workgroup a multiple of 8 (4 waves x row pairs)
    const uint32_t rb_l = (uint32_t)L0.w1->row_bytes;
    struct { uint32_t rows, rb, f16, act, mix, headed, gbase; } jd[ENG_K1_JOBS] = {
        {D, S.rb_d, 0, WRK_ACT_NONE, 0, 1, 0}, {D, S.rb_d, 0, WRK_ACT_NONE, 2, 1, 1}, {D, S.rb_d, 0, WRK_ACT_NONE, 3, 1, 2},
        {S.rw, rb_l, 1, WRK_ACT_TANH, 1, 0, 0}, {S.ra, rb_l, 1, WRK_ACT_NONE, 4, 0, S.rw / 2}, {S.rg, rb_l, 1, WRK_ACT_SIGMOID, 5, 0, (S.rw + S.ra) / 2},
        {S.rv, rb_l, 1, WRK_ACT_NONE, 3, 0, (S.rw + S.ra + S.rg) / 2}};
    double total = 0;
    for (auto& j : jd) total += (double)j.rows * j.rb;
    uint32_t slot1 = 0;
    bool placed = false;
    const uint32_t NK1 = NWG - H;                                      // the head workgroups take no K1 rows (they fetch K2's operands meanwhile)
    for (double target = total / NK1; target < total; target *= 1.03) {
        uint32_t used = 0, worst = 0;
        uint32_t rpw[ENG_K1_JOBS], nw[ENG_K1_JOBS];
        for (int j = 0; j < ENG_K1_JOBS; ++j) {
            uint32_t r = (uint32_t)(target / jd[j].rb);
            r = std::max(2u, r / 2 * 2);
            rpw[j] = r;
            nw[j] = (jd[j].rows + r - 1) / r;
            used += nw[j];
            worst = std::max(worst, std::min(r, jd[j].rows) * jd[j].rb);
        }
        if (used > NK1) continue;
        uint32_t w0 = 0;
        for (int j = 0; j < ENG_K1_JOBS; ++j) {
            S.k1[j] = EngJob{jd[j].rows, jd[j].rb, jd[j].f16, jd[j].act, jd[j].mix, w0, nw[j], rpw[j], jd[j].gbase, jd[j].headed};
            w0 += nw[j];
        }
        slot1 = worst;
        placed = true;
        break;
    }
    if (!placed) { delete e; return no("K1 partition"); }
    S.k3_rpw = std::max(8u, up((D + NWG - 1) / NWG, 8));
    S.k5_rpw = std::max(8u, up((F + NWG - 1) / NWG, 8));
    S.k6_rpw = std::max(2u, up((D + NWG - 1) / NWG, 2));
    if (S.k6_rpw > 32) { delete e; return no("ffn value rows per workgroup"); }
    // ---- LDS
    uint32_t off = 0;
    auto take = [&](uint32_t bytes) { const uint32_t o = off; off += up(bytes, 1024); return o; };
    S.lds_slot1 = take(slot1);
    S.lds_slot5 = take(S.k5_rpw * S.rb_d);
    S.lds_slot6 = take(S.k6_rpw * S.rb_f);
    S.lds_slot3 = take(S.k3_rpw * S.rb_d);
    S.lds_xraw0 = take(D * 2);
    S.lds_xraw1 = take(D * 2);
    const uint32_t naux = S.rw + S.ra + S.rg + S.rv;
    S.lds_ln = take(D * 2);
    S.lds_misc = take(4096);
    S.lds_xs = take(D * 2 + up((naux + 192) * 2, 16) + 1280 * 4);      // a stage's input vector (D elements); K2's scratch lives behind it
    int lds_max = 0;
    hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device);
    if (lds_max < 160 * 1024) lds_max = 160 * 1024;      // gfx950: 160 KiB per workgroup (the attribute reports the 64 KiB default limit on some stacks)
    if (off > (uint32_t)lds_max) { delete e; return no("weights of a layer do not fit the LDS"); }
    // K6's exchange area (the ffn vector, F elements) lies over the xs block, which is dead from K5's rows to the next layer's LN, and
    // over the unused tail behind it: the xs block comes last for that (1.5B: 142 KB in front of it, 11 KB of its own, 16 KB needed)
    S.lds_total = std::max(off, S.lds_xs + F * 2);
    if (S.lds_total > (uint32_t)lds_max) { delete e; return no("the ffn vector's exchange area does not fit the LDS behind a layer's weights"); }
    // ---- granules
    S.g_aux = naux / 2;
    uint32_t g = 0;
    auto gtake = [&](uint32_t n) { const uint32_t o = g; g += up(n, 128); return o; };
    S.g_x = gtake(D / 2);
    S.g_k1 = gtake(S.g_aux + H * 96);
    S.g_o = gtake(D / 2);
    S.g_x1 = gtake(D / 2);
    S.g_k = gtake(F / 2);
    S.g_total = g;
    S.ln_eps = 1.0e-5f; S.gn_eps = 64.0e-5f; S.l2_eps = 1.0e-12f;
    S.rescale = d.rescale ? d.rescale : 0xffffffffu;
    S.state_rows = 64 + 2;

    std::vector<float> hs(m->layers.size() * ENG_NS, 1.0f);
    auto fail_alloc = [&](hipError_t er) { wrk_v7_engine_destroy(e); return wrk_fail(ctx, WRK_E_OOM, "decode engine: %s", hipGetErrorString(er)); };
    hipError_t er;
    std::vector<EngLayer> hl(m->layers.size());
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const auto& L = m->layers[li];
        EngLayer& o = hl[li];
        o.w_r = L.w_r->data; o.w_k = L.w_k->data; o.w_v = L.w_v->data; o.w1 = L.w1->data; o.a1 = L.a1->data; o.g1 = L.g1->data;
        o.v1 = li ? L.v1->data : L.a1->data;
        o.w_o = L.w_o->data; o.ffn_k = L.ffn_w_k->data; o.ffn_v = L.ffn_w_v->data;
        const wrk_matrix* k1m[ENG_K1_JOBS] = {L.w_r, L.w_k, L.w_v, L.w1, L.a1, L.g1, li ? L.v1 : L.a1};
        float* sc = hs.data() + li * ENG_NS;
        for (int j = 0; j < ENG_K1_JOBS; ++j) sc[j] = k1m[j]->out_scale;
        sc[ENG_S_O] = L.w_o->out_scale; sc[ENG_S_FK] = L.ffn_w_k->out_scale; sc[ENG_S_FV] = L.ffn_w_v->out_scale;
    }
    // the f16 vectors of every layer, packed
    if ((er = hipMalloc((void**)&e->vecs, hl.size() * ENG_NV * D * 2)) != hipSuccess) return fail_alloc(er);
    for (size_t li = 0; li < m->layers.size(); ++li) {
        const auto& L = m->layers[li];
        const wrk_buf* src[ENG_NV] = {L.ln1_w, L.ln1_b, L.ln2_w, L.ln2_b, L.x_r, L.x_w, L.x_k, L.x_v, L.x_a, L.x_g, L.w0, L.a0, li ? L.v0 : L.w0,
                                      L.r_k, L.k_k, L.k_a, L.gn_w, L.gn_b, L.ffn_x_k};
        for (int i = 0; i < ENG_NV; ++i) {
            if (!src[i] || src[i]->bytes < (size_t)D * 2) { wrk_v7_engine_destroy(e); return no("a layer vector is missing"); }
            if ((er = hipMemcpy((char*)e->vecs + (li * ENG_NV + i) * (size_t)D * 2, src[i]->ptr, (size_t)D * 2, hipMemcpyDeviceToDevice)) != hipSuccess) return fail_alloc(er);
        }
    }
    // The LoRA up-projections of every layer, packed per head in the order a head workgroup loads them (wrk_lora2_pack.h), once: the rows
    // never change after load.  H x 64 KB per layer at 1.5B (48 MB) beside the matrices themselves, which the launches and prefill keep.
    {
        const EngLora2Ranks R2{S.rw, S.ra, S.rg, S.rv};
        const size_t lb = eng_l2_layer_bytes(R2, H), total_l2 = lb * m->layers.size();
        if ((er = hipMalloc((void**)&e->l2pack, total_l2)) != hipSuccess) {
            (void)hipGetLastError();
            wrk_v7_engine_destroy(e);
            return wrk_fail(ctx, WRK_E_UNSUPPORTED, "decode engine: %zu bytes for the packed LoRA up-projections refused (%s)", total_l2, hipGetErrorString(er));
        }
        std::vector<uint8_t> img(lb), rows[4];
        for (size_t li = 0; li < m->layers.size(); ++li) {
            const auto& L = m->layers[li];
            const wrk_matrix* mats[4] = {L.w2, L.a2, L.g2, li ? L.v2 : nullptr};
            const uint8_t* src[4] = {nullptr, nullptr, nullptr, nullptr};
            size_t rbs[4] = {0, 0, 0, 0};
            for (int i = 0; i < 4; ++i) {
                if (!mats[i]) continue;
                rbs[i] = mats[i]->row_bytes;
                if (rbs[i] < (size_t)eng_l2_rank(R2, i) * 2) { wrk_v7_engine_destroy(e); return no("a LoRA up-projection's rows are shorter than its rank"); }
                rows[i].resize((size_t)D * rbs[i]);
                if ((er = hipMemcpy(rows[i].data(), mats[i]->data, rows[i].size(), hipMemcpyDeviceToHost)) != hipSuccess) return fail_alloc(er);
                src[i] = rows[i].data();
            }
            eng_l2_pack_layer(R2, H, src, rbs, img.data());
            if ((er = hipMemcpy(e->l2pack + li * lb, img.data(), lb, hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(er);
        }
    }
    if ((er = hipMalloc((void**)&e->scal, hs.size() * 4)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMemcpy(e->scal, hs.data(), hs.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMalloc((void**)&e->layers, hl.size() * sizeof(EngLayer))) != hipSuccess) return fail_alloc(er);
    if ((er = hipMemcpy(e->layers, hl.data(), hl.size() * sizeof(EngLayer), hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(er);
    std::vector<uint32_t> hh(2 * NWG, ENG_NO_HEAD);                 // per workgroup: {head or none, rank among the K1 workgroups or none}
    for (uint32_t h = 0; h < H; ++h) hh[2 * ((size_t)h * NWG / H)] = h;
    for (uint32_t w = 0, r = 0; w < NWG; ++w)
        if (hh[2 * w] == ENG_NO_HEAD) hh[2 * w + 1] = r++;
    if ((er = hipMalloc((void**)&e->wg_head, hh.size() * 4)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMemcpy(e->wg_head, hh.data(), hh.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMalloc((void**)&e->gran, (size_t)S.g_total * 8)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMalloc((void**)&e->fail, 256)) != hipSuccess) return fail_alloc(er);
    if ((er = hipMemset(e->fail, 0, 256)) != hipSuccess) return fail_alloc(er);
    const char* tm = getenv("WRK_TIMING");
    if (tm && tm[0] == '1') {
        const size_t n = (size_t)NWG * 16 * 24 * 8 + 64;
        if ((er = hipMalloc((void**)&e->stamps, n)) != hipSuccess) return fail_alloc(er);
        hipMemset(e->stamps, 0, n);
    }
    // compute waves per workgroup: 8 (two per SIMD, <= 168 registers) or 14 (<= 128 registers)
    { const char* ev = getenv("WRK_ENGINE_WAVES"); e->ncw = (ev && atoi(ev) == 14) ? 14 : 8; }
    const void* fn = eng_kernel_fn(e->xd, e->r16, e->ncw);
    // dynamic LDS above 64 KiB needs the attribute (per device: set on every build of an engine)
    if ((er = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.lds_total)) != hipSuccess) {
        wrk_v7_engine_destroy(e);
        return wrk_fail(ctx, WRK_E_UNSUPPORTED, "decode engine: %u bytes of LDS refused (%s)", S.lds_total, hipGetErrorString(er));
    }
    // One workgroup per CU, all of them resident at once.  Checked from the kernel's own resource figures, not with
    // hipOccupancyMaxActiveBlocksPerMultiprocessor: in a process that has ALSO loaded PyTorch's bundled HIP runtime (the test suite imports
    // torch for its gloo tests; bench.py --gpus N for the timing barrier) that call answered 0 blocks without an error for this kernel,
    // while the launches themselves work -- round 3, GPU test run.
    {
        hipFuncAttributes fa{};
        const int waves = e->ncw + 2, per_simd = (waves + 3) / 4;
        if (hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.numRegs > 0) {
            const int alloc = (fa.numRegs + 7) / 8 * 8;
            if (per_simd * alloc > 512 || fa.maxThreadsPerBlock < waves * 64 || (size_t)fa.sharedSizeBytes + S.lds_total > 160 * 1024) {
                const int regs = fa.numRegs;
                wrk_v7_engine_destroy(e);
                return wrk_fail(ctx, WRK_E_UNSUPPORTED, "decode engine: a workgroup of %d waves x %d registers + %u bytes of LDS does not fit a CU", waves, regs,
                                S.lds_total);
            }
        }
        (void)hipGetLastError();
    }
    // LN(ln0) of the whole embedding table, once (round 3): a decode step then starts with the engine itself -- its gather wave takes row
    // `token` of this table -- instead of a gather + LN launch in front of it (4.9 us + a launch boundary per token).  V x D x 2 bytes of HBM.
    // WRK_ENGINE_TABLE=0: off.
    {
        const char* te = getenv("WRK_ENGINE_TABLE");
        if (!(te && te[0] == '0') && m->emb && m->ln0_w && m->ln0_b) {
            const size_t bytes = (size_t)d.num_vocab * D * 2;
            if (hipMalloc(&e->emb_ln, bytes) == hipSuccess) {
                LnMixParams P{};
                P.src = (const f16*)m->emb->ptr; P.ln_w = (const f16*)m->ln0_w->ptr; P.ln_b = (const f16*)m->ln0_b->ptr; P.eps = 1.0e-5f;
                P.d = D; P.nmix = 0; P.ln_out = (f16*)e->emb_ln;
                if (ln_mix(ctx->stream, P, d.num_vocab) != 0 || hipStreamSynchronize(ctx->stream) != hipSuccess) { hipFree(e->emb_ln); e->emb_ln = nullptr; }
            } else e->emb_ln = nullptr;
            (void)hipGetLastError();
        }
    }
    *out = e;
    return WRK_OK;
}

bool wrk_v7_engine_has_table(const wrk_v7_engine* e) { return e && e->emb_ln; }
int wrk_v7_engine_waves(const wrk_v7_engine* e) { return e ? e->ncw : 0; }

void wrk_v7_engine_destroy(wrk_v7_engine* e) {
    if (!e) return;
    if (e->emb_ln) hipFree(e->emb_ln);
    if (e->l2pack) hipFree(e->l2pack);
    if (e->layers) hipFree(e->layers);
    if (e->vecs) hipFree(e->vecs);
    if (e->scal) hipFree(e->scal);
    if (e->wg_head) hipFree(e->wg_head);
    if (e->gran) hipFree(e->gran);
    if (e->fail) hipFree(e->fail);
    if (e->stamps) hipFree(e->stamps);
    delete e;
}

int32_t wrk_v7_engine_enqueue(wrk_v7_engine* e, hipStream_t q, wrk_v7_state* st, uint32_t batch, uint32_t l0, uint32_t l1, const void* x_in, void* x_out,
                              void* v_first, const uint32_t* token) {
    using namespace wrk;
    wrk_ctx* ctx = e->m->ctx;
    EngArgs A{};
    A.S = e->S;
    A.S.layer_begin = l0; A.S.layer_end = l1; A.S.batch = batch;
    A.layers = e->layers; A.vecs = e->vecs; A.l2 = e->l2pack; A.scal = e->scal; A.gran = e->gran; A.x_in = x_in; A.x_out = x_out; A.v_first = v_first;
    if (token && e->emb_ln && l0 == 0) { A.x_in = e->emb_ln; A.x_row = token; }
    A.state = st->data; A.num_batch = st->num_batch; A.fail = e->fail; A.stamps = e->stamps; A.stamp_layer = std::min(5u, l1 - 1);
    // every polled word zeroed before every launch (a memset node, replayed first): tags are > 0 and unique within a launch
    WRK_HIP(ctx, hipMemsetAsync(e->gran, 0, (size_t)e->S.g_total * 8, q));
    const dim3 grid(e->S.nwg), block((e->ncw + 2) * 64);
    hipLaunchKernelGGL(eng_kernel(e->xd, e->r16, e->ncw), grid, block, e->S.lds_total, q, A, (const uint32_t*)e->wg_head);
    WRK_LAUNCH_CHECK(ctx);
    return WRK_OK;
}

int32_t wrk_v7_engine_check(wrk_v7_engine* e) {
    if (!e) return WRK_OK;
    wrk_ctx* ctx = e->m->ctx;
    uint32_t f = 0;
    WRK_HIP(ctx, hipMemcpy(&f, e->fail, 4, hipMemcpyDeviceToHost));
    if (f) {
        hipMemset(e->fail, 0, 4);
        return wrk_fail(ctx, WRK_E_HIP, "decode engine: a hand-off wait gave up (stage mask 0x%x): workgroups not co-resident or a producer died", f);
    }
    return WRK_OK;
}

void wrk_v7_engine_report(wrk_v7_engine* e) {
    using namespace wrk;
    if (!e || !e->stamps) return;
    const uint32_t NWG = e->S.nwg, NW = (uint32_t)e->ncw + 2;
    std::vector<unsigned long long> h((size_t)NWG * NW * 24);
    if (hipMemcpy(h.data(), e->stamps, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    unsigned long long t0 = ~0ull;
    for (auto v : h) if (v && v < t0) t0 = v;
    std::vector<char> is_head(NWG, 0);                      // the placement of wrk_v7_engine_create
    for (uint32_t hd = 0; hd < e->S.H; ++hd) is_head[(size_t)hd * NWG / e->S.H] = 1;
    // wave: which wave's stamp; -1 = the LAST compute wave of each workgroup to pass the point.  cls: 0 = workgroups without a head,
    // 1 = head workgroups, -1 = all
    auto col = [&](int wave, uint32_t k, const char* label, int cls = -1) {
        std::vector<double> v;
        for (uint32_t w = 0; w < NWG; ++w) {
            if (cls >= 0 && is_head[w] != cls) continue;
            unsigned long long x = 0;
            if (wave >= 0) x = h[((size_t)w * NW + wave) * 24 + k];
            else for (int cw = 0; cw < e->ncw; ++cw) x = std::max(x, h[((size_t)w * NW + cw) * 24 + k]);
            if (x) v.push_back((double)(x - t0) * 0.01);
        }
        if (v.empty()) return;
        std::sort(v.begin(), v.end());
        fprintf(stderr, "  %-62s %4zu WGs  first %7.2f  median %7.2f  last %7.2f us\n", label, v.size(), v.front(), v[v.size() / 2], v.back());
    };
    {
        unsigned long long tail[2] = {0, 0};
        if (hipMemcpy(tail, e->stamps + (size_t)NWG * 16 * 24, 16, hipMemcpyDeviceToHost) == hipSuccess && tail[1])
            fprintf(stderr, "[WRK_TIMING] decode engine: shader clock over the last launch %.0f MHz (%llu cycles in %.1f us)\n",
                    (double)tail[0] / ((double)tail[1] * 0.01), tail[0], (double)tail[1] * 0.01);
    }
    const int G = e->ncw, Ld = e->ncw + 1;
    fprintf(stderr, "[WRK_TIMING] decode engine (%d compute waves), one layer of the last token; us since the layer's first stamp\n", e->ncw);
    col(G, 0, "gather: layer input complete, workgroups without a head", 0);
    col(G, 0, "gather: layer input complete, head workgroups", 1);
    col(-1, 19, "operand requests issued, slowest wave, head workgroups", 1);
    col(0, 1, "K1 start (input + weights in LDS), wave 0, no head", 0);
    col(0, 1, "K1 start (input in LDS), wave 0, head workgroups", 1);
    col(0, 2, "K1 LN + shift done, wave 0");
    col(0, 3, "K1 rows published, wave 0, no head", 0);
    col(-1, 3, "K1 rows published, slowest wave, no head", 0);
    col(-1, 3, "K1 LN + shift done, slowest wave, head workgroups", 1);
    col(G, 4, "gather (heads): LoRA intermediates complete");
    col(G, 1, "gather (heads): K1 outputs complete");
    col(0, 4, "K2 start");
    col(-1, 16, "K2 LoRA dots done, slowest wave");
    col(0, 17, "K2 per-channel stage done");
    col(-1, 18, "K2 state updated, slowest wave");
    col(0, 5, "K2 published");
    col(G, 2, "gather: head outputs complete");
    col(0, 6, "K3 start");
    col(-1, 7, "K3 published, slowest wave");
    col(G, 3, "gather: x1 complete");
    col(0, 8, "K5 start");
    col(0, 14, "K5 LN + shift done, wave 0");
    col(0, 9, "K5 published, wave 0");
    col(-1, 9, "K5 published, slowest wave");
    col(0, 10, "K6 own quarter of the ffn vector swept, wave 0");
    col(-1, 10, "K6 swept, slowest wave");
    col(0, 11, "K6 start");
    col(-1, 15, "K6 inputs read back from LDS, slowest wave");
    col(-1, 12, "K6 partial sums done, slowest wave");
    col(0, 13, "K6 published");
    col(Ld, 0, "loader: K1 slot free, next layer's fill issued");
}
