// MXFP4 on gfx950: the OCP microscaling FP4 -- 32 e2m1 codes under one power-of-two E8M0 scale -- is the one 4-bit
// format the hardware decodes itself.  v_cvt_scalef32_pk_f16_fp4 turns the two codes of a byte into two f16 values; at unit scale they are
// exactly the e2m1 values {0, .5, 1, 1.5, 2, 3, 4, 6} with their sign.  A block is 32 elements, the K of v_mfma_f32_16x16x32_f16.  Every
// kernel here keeps the block scale OUT of the f16 domain: a block's 32 products are summed in f32 from exact f16 x f16 products, and that
// sum is multiplied by 2^(e - 127) in f32, the factor built from e with integer ops.  That is exact for every e (0 gives the subnormal
// 2^-127, 255 gives +inf, the f32 overflow of 2^128), where a scale folded into f16 weights is not.
//
//   mx_matvec_kernel   1 .. 4 tokens per pass, f16 inputs.  A lane owns one block per step: one 16-byte code load, one scale byte, 16
//                      conversions, then per token 16 packed dot products against inputs staged in LDS as f16, and one f32 multiply.
//                      Two rows share every input fragment a lane reads.  Short rows (K < 8192): the four waves of a workgroup take
//                      different rows; long rows: the four waves split a row's blocks, 256 per step, and the partial sums meet in LDS.
//                      The epilogue (activation, output scale, residual, store, arg-max partial) runs once per (row, token) from LDS.
//   mx_matvec_f32_kernel   f32 inputs (Bundle::<f32> frames): codes widened to f32, fma in f32, one wave per row -- a correctness path.
//   mx_gemm_kernel     5 tokens and more: v_mfma_f32_16x16x32_f16 with a zero accumulator per block, then total += 2^(e - 127) * acc for
//                      the four rows a lane holds (per-row accumulator scaling).  A wave owns a 16-row tile over all of K and up to 64
//                      tokens; the A fragment of a lane is one dword of the block, its B fragment 16 bytes of the token's row.
//   mx_quant_kernel    f16 -> MXFP4 by the OCP MX rule, one thread per block, straight into the stored layout.
#include "wrk_matvec_dev.h"
#include "wrk_gemm_route.h"
#include "wrk_mxfp4.h"

namespace wrk {

typedef float mx_f32x4 __attribute__((ext_vector_type(4)));

// 2^(e - 127) for every E8M0 byte, from integer ops: the byte is the f32 exponent field; 0 is the subnormal 2^-127, 255 is +inf
__device__ __forceinline__ float mx_scale(uint32_t e) { return __builtin_bit_cast(float, e ? e << 23 : 0x00400000u); }

// the two codes of byte SEL of a dword -> two f16 (element order: low nibble first), exactly the e2m1 values
template <int SEL>
__device__ __forceinline__ f16x2 mx_cvt(uint32_t q) { return __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(q, 1.0f, SEL); }

// the 8 codes of a dword -> f16x8, element i from bits 4i .. 4i + 3
__device__ __forceinline__ f16x8 mx_cvt8(uint32_t q) {
    const f16x2 a = mx_cvt<0>(q), b = mx_cvt<1>(q), c = mx_cvt<2>(q), d = mx_cvt<3>(q);
    f16x8 r = {a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    return r;
}

// sum of 8 exact f16 x f16 products, added to acc in f32
__device__ __forceinline__ float mx_dot8(uint32_t q, f16x8 x, float acc) {
    acc = __builtin_amdgcn_fdot2(mx_cvt<0>(q), __builtin_shufflevector(x, x, 0, 1), acc, false);
    acc = __builtin_amdgcn_fdot2(mx_cvt<1>(q), __builtin_shufflevector(x, x, 2, 3), acc, false);
    acc = __builtin_amdgcn_fdot2(mx_cvt<2>(q), __builtin_shufflevector(x, x, 4, 5), acc, false);
    acc = __builtin_amdgcn_fdot2(mx_cvt<3>(q), __builtin_shufflevector(x, x, 6, 7), acc, false);
    return acc;
}

__device__ __forceinline__ const JobDev& mx_job(const MatvecParams& P) {
    int ji = 0;
#pragma unroll
    for (int q = 1; q < MAX_JOBS; ++q)
        if (q < P.njobs && blockIdx.x >= P.jobs[q].wg_begin) ji = q;
    return P.jobs[ji];
}

// ------------------------------------------------------------------ decode matvec, f16 inputs
constexpr uint32_t MX_MAX_RPW = 32;         // rows of a workgroup (matvec_num_wg never gives more)
constexpr uint32_t MX_KSPLIT_BLOCKS = 256;  // rows of this many blocks and more are split over the four waves

template <int NT>
__global__ void __launch_bounds__(256) mx_matvec_kernel(const MatvecParams P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_smem[];
    constexpr int R = 2;                            // rows that share an input fragment
    const JobDev& J = mx_job(P);
    const uint32_t K = J.k, nblk = K >> 5;
    f16* xs = (f16*)mx_smem;                                        // [NT][K]
    float* part = (float*)(mx_smem + (size_t)NT * K * 2);           // [MX_MAX_RPW][NT][4 waves]
    const uint32_t ntok = J.in.shape[1] * J.in.shape[2];
    const uint32_t tok0 = blockIdx.y * NT;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r0 = (blockIdx.x - J.wg_begin) * J.rows_per_wg;
    const uint32_t nrows = min(min(r0 + J.rows_per_wg, J.m) - r0, MX_MAX_RPW);
    const bool ksplit = nblk >= MX_KSPLIT_BLOCKS;

    // inputs -> LDS as f16 (dead token slots: zeros)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
        const uint32_t tk = tok0 + n;
        const bool live = tk < ntok;
        const uint32_t t = live ? tk % J.in.shape[1] : 0, b = live ? tk / J.in.shape[1] : 0;
        const size_t base = dt_index(J.in, 0, t, b);
        f16* xd = xs + (size_t)n * K;
        if (J.in.dtype == WRK_F16 && (base & 7u) == 0) {
            const f16x8* src = (const f16x8*)((const f16*)J.in.p + base);
            const f16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
            for (uint32_t v = tid; v < (K >> 3); v += 256) ((f16x8*)xd)[v] = live ? src[v] : zero;
        } else {
            for (uint32_t i = tid; i < K; i += 256) xd[i] = live ? (f16)dt_load(J.in, base + i) : (f16)0.0f;
        }
    }
    __syncthreads();

    // short rows: wave w owns rows w, w + 4, ... and walks all blocks, 64 per step; long rows: every wave walks every row, wave w the
    // blocks 64w + lane + 256i
    const uint32_t rstart = ksplit ? 0u : wave, rstep = ksplit ? 1u : 4u;
    const uint32_t cstart = ksplit ? tid : lane, cstep = ksplit ? 256u : 64u;
    const uint32_t slot = ksplit ? wave : 0u;
    for (uint32_t ri = rstart; ri < nrows; ri += R * rstep) {       // wave-uniform trip count
        float acc[R][NT];
#pragma unroll
        for (int rb = 0; rb < R; ++rb)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[rb][n] = 0.0f;
        for (uint32_t c = cstart; c < nblk; c += cstep) {
            u32x4 q[R];
            float sc[R];
#pragma unroll
            for (int rb = 0; rb < R; ++rb) {
                const uint32_t row = min(ri + rb * rstep, nrows - 1);       // a missing second row repeats the last one; never stored
                const uint8_t* wr = J.w + (size_t)(r0 + row) * J.row_bytes;
                q[rb] = __builtin_nontemporal_load((const u32x4*)(wr + (size_t)c * 16));
                sc[rb] = mx_scale(wr[(K >> 1) + c]);
            }
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const f16x8* xp = (const f16x8*)(xs + (size_t)n * K + (size_t)c * 32);
                const f16x8 x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
#pragma unroll
                for (int rb = 0; rb < R; ++rb) {
                    float p = mx_dot8(q[rb].x, x0, 0.0f);
                    p = mx_dot8(q[rb].y, x1, p);
                    p = mx_dot8(q[rb].z, x2, p);
                    p = mx_dot8(q[rb].w, x3, p);
                    acc[rb][n] += p * sc[rb];
                }
            }
        }
#pragma unroll
        for (int rb = 0; rb < R; ++rb) {
            const uint32_t row = ri + rb * rstep;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float v = wave_sum(acc[rb][n]);
                if (lane == 0 && row < nrows) part[((size_t)row * NT + n) * 4 + slot] = v;
            }
        }
    }
    __syncthreads();

    // one thread per (row, token): combine, activation, residual, store; the stored value stays in LDS for the arg-max
    for (uint32_t idx = tid; idx < nrows * NT; idx += 256) {
        const uint32_t row = idx / NT, n = idx % NT, tk = tok0 + n;
        const float* p = part + (size_t)idx * 4;
        const float v = ksplit ? (p[0] + p[1]) + (p[2] + p[3]) : p[0];
        float o = -3.0e38f;
        if (tk < ntok) {
            const uint32_t t = tk % J.in.shape[1], b = tk / J.in.shape[1], r = r0 + row;
            o = act_apply(J.act, v * J.scale);
            if (J.has_res) o = dt_round(J.out, o) + dt_load(J.res, dt_index(J.res, r, t, b));
            dt_store(J.out, dt_index(J.out, r, t, b), o);
        }
        part[(size_t)idx * 4] = o;
    }
    if (J.amax_val) {       // fused greedy sampling, stage 1: (max, first row) of the rows this workgroup produced, per token
        __syncthreads();
        if (tid < NT && tok0 + tid < ntok) {
            float bv = -3.0e38f;
            uint32_t bi = 0xffffffffu;
            for (uint32_t row = 0; row < nrows; ++row) {
                const float o = part[((size_t)row * NT + tid) * 4];
                if (o > bv) { bv = o; bi = r0 + row; }
            }
            const size_t at = (size_t)(blockIdx.x - J.wg_begin) * ntok + tok0 + tid;
            J.amax_val[at] = bv;
            J.amax_idx[at] = bi;
        }
    }
}

// ------------------------------------------------------------------ decode matvec, f32 inputs
__global__ void __launch_bounds__(256) mx_matvec_f32_kernel(const MatvecParams P) {
    const JobDev& J = mx_job(P);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t K = J.k, nblk = K >> 5;
    const uint32_t r0 = (blockIdx.x - J.wg_begin) * J.rows_per_wg, r1 = min(r0 + J.rows_per_wg, J.m);
    const uint32_t tk = blockIdx.y, t = tk % J.in.shape[1], b = tk / J.in.shape[1];
    const size_t xbase = dt_index(J.in, 0, t, b);
    for (uint32_t r = r0 + wave; r < r1; r += 4) {      // wave-uniform
        const uint8_t* wr = J.w + (size_t)r * J.row_bytes;
        float acc = 0.0f;
        for (uint32_t c = lane; c < nblk; c += 64) {
            const u32x4 q = *(const u32x4*)(wr + (size_t)c * 16);
            const uint32_t qd[4] = {q.x, q.y, q.z, q.w};
            float p = 0.0f;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const f16x8 w8 = mx_cvt8(qd[d]);
#pragma unroll
                for (int i = 0; i < 8; ++i) p = __builtin_fmaf((float)w8[i], dt_load(J.in, xbase + (size_t)c * 32 + d * 8 + i), p);
            }
            acc += p * mx_scale(wr[(K >> 1) + c]);
        }
        const float v = wave_sum(acc);
        if (lane == 0) {
            float o = act_apply(J.act, v * J.scale);
            if (J.has_res) o = dt_round(J.out, o) + dt_load(J.res, dt_index(J.res, r, t, b));
            dt_store(J.out, dt_index(J.out, r, t, b), o);
        }
    }
}

int mxfp4_matvec(hipStream_t s, const MatvecParams& P, uint32_t total_wg, uint32_t ntok, bool dry) {
    bool f32in = false;
    uint32_t kmax = 0;
    for (int j = 0; j < P.njobs; ++j) {
        const JobDev& J = P.jobs[j];
        if (J.kind != WRK_MAT_MXFP4 || (J.k & 31u) || J.rows_per_wg > MX_MAX_RPW) return -1;
        if (J.pro || J.carry_dst || J.gate) return -3;      // the fused decode prologue / carry / gate live in the dmv kernels: the caller's 7-launch layer
        f32in = f32in || J.in.dtype == WRK_F32;
        kmax = J.k > kmax ? J.k : kmax;
    }
    if (f32in) {
        for (int j = 0; j < P.njobs; ++j)
            if (P.jobs[j].amax_val) return -3;
        if (!dry) hipLaunchKernelGGL(mx_matvec_f32_kernel, dim3(total_wg, ntok), dim3(256), 0, s, P);
        return 0;
    }
    // tokens per pass: as many as the staged inputs leave room for in 64 KiB of LDS, at most 4
    const size_t tail = (size_t)MX_MAX_RPW * 4 * 4 * 4;
    int nt = ntok >= 3 ? 4 : (int)ntok;
    while (nt > 1 && (size_t)nt * kmax * 2 + tail > 64 * 1024) nt >>= 1;
    const size_t smem = (size_t)nt * kmax * 2 + tail;
    if (smem > 160 * 1024) return -1;
    if (dry) return 0;
    void (*fn)(const MatvecParams) = nt == 4 ? mx_matvec_kernel<4> : (nt == 2 ? mx_matvec_kernel<2> : mx_matvec_kernel<1>);
    if (smem > 64 * 1024 && hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return -1;
    hipLaunchKernelGGL(fn, dim3(total_wg, (ntok + nt - 1) / nt), dim3(256), smem, s, P);
    return 0;
}

// ------------------------------------------------------------------ prefill GEMM
struct MxGemmJob {
    const uint8_t* w;
    const f16* x;               // dense token stacks: token tok at base + tok * stride (elements)
    void* out_p;
    const void* res_p;
    uint32_t k, m, n, row_bytes, act, has_res;
    uint32_t xs, os, rs, out32, res32;
    float scale;
};

// A wave: rows m0 .. m0 + 15 over all of K, token tiles n0 + 16t (t < NT).  Lane (r = lane & 15, g = lane >> 4) feeds the matrix core row
// r's elements 8g .. 8g + 7 of the block (one dword) and token r's inputs of the same k, and receives rows 4g .. 4g + 3 of token column r.
template <int NT>
__global__ void __launch_bounds__(256) mx_gemm_kernel(const MxGemmJob P) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t r = lane & 15, g = lane >> 4;
    const uint32_t m0 = (blockIdx.x * (blockDim.x >> 6) + wave) * 16;
    if (m0 >= P.m) return;                                  // whole waves leave; no barrier below
    const uint32_t n0 = blockIdx.y * 16 * NT;
    const uint32_t K = P.k, nblk = K >> 5;
    const uint8_t* wrow = P.w + (size_t)min(m0 + r, P.m - 1) * P.row_bytes + 4 * g;
    const uint8_t* srow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) srow[i] = P.w + (size_t)min(m0 + 4 * g + i, P.m - 1) * P.row_bytes + (K >> 1);
    const f16* xrow[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) xrow[t] = P.x + (size_t)min(n0 + 16 * t + r, P.n - 1) * P.xs + 8 * g;      // a dead column is computed, never stored

    mx_f32x4 total[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) total[t] = (mx_f32x4){0.f, 0.f, 0.f, 0.f};

    // four blocks per trip: four code dwords and, per row of the lane, one dword of four scale bytes (the scale plane is padded to 16 bytes,
    // so the last trip's dword stays inside the row); blocks past the row's end are skipped, uniformly over the wave
    for (uint32_t s0 = 0; s0 < nblk; s0 += 4) {
        const uint32_t cnt = min(4u, nblk - s0);
        uint32_t q[4], e4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) q[u] = *(const uint32_t*)(wrow + (size_t)min(s0 + u, nblk - 1) * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i) e4[i] = *(const uint32_t*)(srow[i] + s0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((uint32_t)u >= cnt) break;
            const f16x8 a = mx_cvt8(q[u]);
            float sc[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[i] = mx_scale((e4[i] >> (8 * u)) & 255u);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f16x8 bf = *(const f16x8*)(xrow[t] + (size_t)(s0 + u) * 32);
                const mx_f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bf, (mx_f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) total[t][i] = __builtin_fmaf(sc[i], acc[i], total[t][i]);
            }
        }
    }

    // store: rows m0 + 4g + (0..3) of token column r of each tile (M % 4 == 0: the four rows are all inside or all outside)
    const uint32_t mr = m0 + 4 * g;
    if (mr >= P.m) return;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const uint32_t tok = n0 + 16 * t + r;
        if (tok >= P.n) continue;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = act_apply(P.act, total[t][i] * P.scale);
            if (P.has_res) {
                const size_t ro = (size_t)tok * P.rs + mr + i;
                o[i] = (P.out32 ? o[i] : r16(o[i])) + (P.res32 ? ((const float*)P.res_p)[ro] : (float)((const f16*)P.res_p)[ro]);
            }
        }
        const size_t oo = (size_t)tok * P.os + mr;
        if (P.out32) *(mx_f32x4*)((float*)P.out_p + oo) = (mx_f32x4){o[0], o[1], o[2], o[3]};
        else { typedef _Float16 f16x4 __attribute__((ext_vector_type(4))); *(f16x4*)((f16*)P.out_p + oo) = (f16x4){(f16)o[0], (f16)o[1], (f16)o[2], (f16)o[3]}; }
    }
}

static bool mx_gemm_ok(const MatJob& j, uint32_t n, uint32_t min_tokens) {
    if (j.kind != WRK_MAT_MXFP4 || j.in.shape[1] * j.in.shape[2] != n || n < min_tokens) return false;
    if (!dense_stack(j.in) || !dense_stack(j.out) || (j.has_res && !dense_stack(j.res))) return false;
    if (j.m < 4 || (j.m & 3u) || (j.k & 31u) || j.k < 32 || j.in.dtype != WRK_F16) return false;
    if (j.has_res && j.res.dtype != WRK_F16 && j.res.dtype != WRK_F32) return false;
    if (j.out.dtype != WRK_F16 && j.out.dtype != WRK_F32) return false;
    // four consecutive output rows go out as one vector; a lane's B fragment is one 16-byte load
    if ((stack_base(j.out) | j.out.stride[0]) & 3u) return false;
    if ((j.in.stride[0] & 7u) || (j.in.offset[0] & 7u)) return false;
    return true;
}

int mxfp4_gemm(hipStream_t s, const MatJob* jobs, int njobs, uint32_t min_tokens, int num_cu) {
    if (njobs <= 0) return -2;
    const uint32_t n = jobs[0].in.shape[1] * jobs[0].in.shape[2];
    for (int q = 0; q < njobs; ++q)
        if (!mx_gemm_ok(jobs[q], n, min_tokens)) return -2;
    for (int q = 0; q < njobs; ++q) {
        const MatJob& j = jobs[q];
        MxGemmJob P;
        P.w = j.w; P.k = j.k; P.m = j.m; P.n = n; P.row_bytes = j.row_bytes; P.act = j.act; P.has_res = j.has_res; P.scale = j.scale;
        P.x = (const f16*)j.in.p + stack_base(j.in); P.xs = j.in.stride[0];
        P.out32 = j.out.dtype == WRK_F32; P.os = j.out.stride[0];
        P.out_p = (char*)j.out.p + stack_base(j.out) * (P.out32 ? 4 : 2);
        P.res32 = j.has_res && j.res.dtype == WRK_F32; P.rs = j.has_res ? j.res.stride[0] : 0;
        P.res_p = j.has_res ? (const char*)j.res.p + stack_base(j.res) * (P.res32 ? 4 : 2) : nullptr;
        // token tiles per wave: 16, 32 or 64 tokens; waves per workgroup: four (they share the tokens' rows in the caches) unless that
        // leaves CUs idle, then one
        const uint32_t nt = n <= 16 ? 1 : (n <= 32 ? 2 : 4);
        const uint32_t ty = (n + 16 * nt - 1) / (16 * nt), tiles = (j.m + 15) / 16;
        const uint32_t wpw = (uint64_t)((tiles + 3) / 4) * ty >= 2u * (uint32_t)(num_cu > 0 ? num_cu : 1) ? 4u : 1u;
        const dim3 grid((tiles + wpw - 1) / wpw, ty), block(64 * wpw);
        if (nt == 1) mx_gemm_kernel<1><<<grid, block, 0, s>>>(P);
        else if (nt == 2) mx_gemm_kernel<2><<<grid, block, 0, s>>>(P);
        else mx_gemm_kernel<4><<<grid, block, 0, s>>>(P);
    }
    return 0;
}

// ------------------------------------------------------------------ quantiser
// One thread per block of 32: amax, e = clamp(floor(log2 amax) - 2 + 127, 0, 254) read off amax's f32 exponent field, then every element
// times 2^(127 - e) (exact: a power of two, nothing leaves the normal f32 range) to the nearest e2m1 value, ties to the even code.
__global__ void __launch_bounds__(256) mx_quant_kernel(const f16* __restrict__ src, uint8_t* __restrict__ dst, uint32_t k, uint32_t m, uint32_t row_bytes) {
    const uint32_t nblk = k >> 5;
    const size_t blk = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= (size_t)nblk * m) return;
    const uint32_t row = (uint32_t)(blk / nblk), b = (uint32_t)(blk % nblk);
    const f16x8* sp = (const f16x8*)(src + (size_t)row * k + (size_t)b * 32);
    const f16x8 v[4] = {sp[0], sp[1], sp[2], sp[3]};
    float amax = 0.0f;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf((float)v[d][i]));
    uint8_t* out = dst + (size_t)row * row_bytes;
    uint32_t e = 0;
    u32x4 codes = {0u, 0u, 0u, 0u};
    if (amax > 0.0f) {
        const int ex = (int)((__builtin_bit_cast(uint32_t, amax) >> 23) & 255u) - 2;       // f16 values are normal in f32: the field is floor(log2) + 127
        e = (uint32_t)(ex < 0 ? 0 : (ex > 254 ? 254 : ex));
        const float inv = __builtin_bit_cast(float, (254u - e) << 23);                      // 2^(127 - e); e >= 101 here
        uint32_t cd[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            cd[d] = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float w = (float)v[d][i];
                const float a = fabsf(w) * inv;
                // midpoints of {0, .5, 1, 1.5, 2, 3, 4, 6}; a tie goes to the even code: up into 2, 4, 6, down onto 0, 2, 4, 6
                const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                                   (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
                const uint32_t sign = (__builtin_bit_cast(uint32_t, w) >> 31) << 3;
                cd[d] |= (c | sign) << (4 * i);
            }
        }
        codes = (u32x4){cd[0], cd[1], cd[2], cd[3]};
    }
    *(u32x4*)(out + (size_t)b * 16) = codes;
    out[(k >> 1) + b] = (uint8_t)e;
}

void quantize_mxfp4(hipStream_t s, const void* src_f16, uint8_t* dst, uint32_t k, uint32_t m, uint32_t row_bytes) {
    const size_t blocks = (size_t)(k >> 5) * m;
    hipLaunchKernelGGL(mx_quant_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, (const f16*)src_f16, dst, k, m, row_bytes);
}

}  // namespace wrk
