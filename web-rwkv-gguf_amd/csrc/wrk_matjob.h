// The two plain structures a matmul launch is described by, free of HIP: the launchers (wrk_matvec.hip, wrk_gemm.hip), the routing
// planner (wrk_gemm_route.h) and the host tests of the planner share them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "wrk_hip.h"

// ------------------------------------------------------------------ device-side tensor descriptor
// Mirrors `View` addressing (see wrk_hip.h).  Passed by value to kernels.
struct DTensor {
    void* p;
    uint32_t dtype;     // WRK_F16 / WRK_F32
    uint32_t shape[4];
    uint32_t stride[4];
    uint32_t offset[4];
};

namespace wrk {

struct MatJob {
    const uint8_t* w;       // matrix data (device layout)
    const uint8_t* aux;
    uint32_t kind, flags;
    uint32_t k, m;
    uint32_t row_bytes;
    DTensor in;             // [K, T, B]
    DTensor out;            // [M, T, B]
    uint32_t act;
    uint32_t sparse;
    uint32_t has_res = 0;   // fused `add`: out = round_to_out_dtype(act(W.x)) + res
    DTensor res{};
    float* amax_val = nullptr;      // optional fused arg-max partials [num_wg][ntok]
    uint32_t* amax_idx = nullptr;
    // fused decode prologue / epilogue (single input vector only; matvec() returns -3 if it cannot honour them)
    uint32_t pro = 0;               // 1: input = mix(LN(in; ln_w, ln_b, pro_eps), prev, mixw)
                                    // 2: input = mixw * r16(r16(GN64(in; ln_w, ln_b, pro_eps)) + prev): the post-WKV stage of a split head
                                    //    (in = WKV output, prev = f32 time_first term, mixw = gate), dmv kernels only
    float pro_eps = 0.0f;
    const void *ln_w = nullptr, *ln_b = nullptr, *mixw = nullptr;
    const float* prev = nullptr;    // f32 shift-state row of this sequence
    void* ln_out = nullptr;         // f16 [K]: LN(in), published by the first workgroup of the job
    const void* carry_src = nullptr;    // epilogue: carry_dst[row] = carry_src[row]
    float* carry_dst = nullptr;
    float scale = 1.0f;                 // wrk_matrix::out_scale
    const void* gate = nullptr;         // f16 [M]: out = round(sigmoid(gate[row]) * round(act(W.x)))  (channel_mix.wgsl:104-106, RWKV-6), before the residual
    unsigned long long* dbg = nullptr;  // WRK_TIMING=1: 16 device timestamps of this launch (first and last workgroup)
    // several input vectors (2 .. 4 sequences decoding together, dmv kernels): element strides from one token's operand to the next
    uint32_t tok_prev_stride = 0, tok_mix_stride = 0, tok_carry_src_stride = 0, tok_carry_dst_stride = 0, tok_gate_stride = 0;
    // decode batches on the matrix cores: scratch of the K-sliced GEMM (f32 partial tiles, per-row-group arrival counters that are
    // zero between launches); taken from the first job of a launch, nullptr = the kernel is not used
    float* ks_part = nullptr;
    uint32_t* ks_cnt = nullptr;
    size_t ks_part_cap = 0;         // floats
    uint32_t ks_cnt_cap = 0;
    // third-generation prefill tile (>= 512 stacked tokens, Q4_K): scratch for the sub-block input sums, taken from the first job of a
    // launch (wrk_ctx::gemm_scratch); nullptr = the kernel is not used
    void* xsum = nullptr;
    size_t xsum_cap = 0;            // bytes
};

}  // namespace wrk
