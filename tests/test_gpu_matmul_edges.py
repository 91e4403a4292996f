"""Every matmul kernel on the full range of block encodings and inputs (C ABI wrk_op_matmul, `wrk.Matrix(...).matmul_op`).

The other GPU matmul tests multiply quantiser output (oracle/quantize.py: d > 0, scales clipped away from 0 and -128, Gaussian codes) with
N(0, 1) inputs.  Here the weights are raw blocks written byte by byte (tests/blocks_ref.py: `uniform_bytes`, `extreme_codes`, `signed`,
`d_range`) and the inputs come in six profiles (`normal`, `large`, `large_same_sign`, `tiny`, `sparse`, `cancelling`); the reference is
the f64 contraction of the oracle-decoded weights (pinned to a scalar decoder by tests/test_blocks_ref.py).

Bound, every case, no per-case override and NO additive floor (a floor would make `tiny` vacuous):
    |got - want| <= C * (terms_abs @ |x|),   C = 4e-6
`terms_abs` is the sum of the absolute values of the terms of a weight's decode formula (|d sc q| + |dmin m| for Q4_K / Q5_K): the
kernels factor the min term out, so their rounding error scales with the parts.  C is tied to a reference in test_blocks_ref.py (an f32
accumulation in 16-wide partial sums stays below C / 2 on every input profile at K = 16384).  In addition: every output is finite
(all expected values here are far inside the f32 range); an all-zero token gives exactly 0.0; the value-preserving sign flips of Q6_K and
Q8_0 (blocks_ref.flip) give the same f32 bits wherever the kernel is sign-symmetric (see BIT_IDENTICAL) and stay inside the bound elsewhere.

Which kernel a case runs on follows from its shape and from the switches that are read per call.  wrk_op_matmul (wrk_api.hip) sends
turbo calls of >= 2 tokens to matmul_mfma, whose routing is one pure function, gemm_plan (web-rwkv-gguf_amd/csrc/wrk_gemm_route.h); every
other call, and a launch gemm_plan declines, goes to matvec (wrk_matvec.hip, wrk_dmv.hip launch_dmv).  tests/matmul_paths.py holds the shapes
and names each turbo path's route; tests/test_gemm_route_host.py asserts on the CPU that gemm_plan gives every row that route, so the
table below cannot drift from the dispatch:

| path        | kernel                                   | rule the shape relies on                                                                  |
|-------------|------------------------------------------|-------------------------------------------------------------------------------------------|
| vec1        | dmv_kernel (NF4, long ROUND_F16 rows: matvec_kernel family) | T = 1, turbo off; K = 256 / 512 (one chunk) and K = 8192 (4096 F16): K over the waves, two iterations; MATRIX_EXACT and MATRIX_ROUND_F16 |
| vecT        | dmv token kernels, matvec kernels (Q8_0, INT8, NF4) | T = 2, 3, 4, turbo off (launch_dmv: <= 4 tokens; Q8_0 / Int8 / NF4 fall back)              |
| ks14        | gemm_kernel<1,4>                         | turbo, T = 5 <= 16, wg < 256 but K = 512 < 4096: not deep                              |
| ks18        | gemm_kernel<1,8>                         | turbo, T = 16, 4 row tiles, K = 4096: deep                                                |
| ks24        | gemm_kernel<2,4>                         | turbo, T = 17 (16 < n <= 64), K = 512                                                     |
| ks28        | gemm_kernel<2,8>                         | turbo, T = 40 < 48 (no tile), K = 4096: deep                                              |
| ks44        | gemm_kernel<4,4>                         | turbo, T = 100 > 64, m = 32 < 64 rows: no tile kernel                                     |
| pair        | gemm_pair_kernel                         | WRK_GEMM_PAIR=1, m = 6416 (401 row tiles >= 400), T = 5 / 16, K = 512; Q4_K / Q5_K / F16  |
| tile1       | gemm_tile_kernel                         | T = 100 (48 <= n < 128: not tile3, < 512: not tile2), 33 x 2 = 66 tiles >= 64 at K <= 2560 |
| tile2       | gemm_tile2_kernel                        | T = 520 >= 512, 9 x 9 tiles, K % 128 == 0: Q8_0, F16; Q4_K / Q5_K with WRK_GEMM_TILE3=0   |
| tile2_q8_48 | gemm_tile2_kernel                        | Q8_0 from 48 tokens: T = 48, 65 tiles at K = 256                                          |
| tile3       | xsum_kernel + gemm_tile3_kernel          | T = 515 >= 512, Q4_K / Q5_K, m = 132 >= 128; K = 2048 (sum pre-pass: a wave per token), 2560 (last group of two blocks), 8192 |
| tile3_split | xsum + gemm_tile3 (grid.z) + t3_reduce_kernel | T = 140 (128 < n <= 256) K = 8192, and T = 128 with K = 4096 (gemm_plan_tile3)              |
| plane_vec / plane_mfma | matvec kernels / gemm_kernel<2,4> | INT8, NF4: T = 1, 3 turbo off; T = 33 turbo (as test_gpu_wrkquant.py)                     |

profiles/matmul_edges_kernel_stats.csv is a rocprofv3 --kernel-trace --stats run of this file and lists every kernel of the table.

All encoding x input pairs run on every path for every kind the path supports (nothing is paired or thinned).  Outputs are f32 for the
input crossing (an f16 store of a huge result overflows legitimately); the f16-output + activation epilogue is crossed with the encoding
profiles on `normal` inputs.

What this file found (MI355X): see DESIGN.md, "Value range".
"""
import functools

import numpy as np
import pytest

import blocks_ref as br
import wrk
from oracle import dequant as dq
from matmul_paths import PATHS
from oracle import wrkquant as wq

pytestmark = pytest.mark.gpu

C = 4e-6
F16_LONG = {8192: 4096}                     # F16 rows: the two-iteration walk starts at 4096


def shapes_of(path, kind):
    out = []
    for k, m, T in PATHS[path][1]:
        if kind == "F16" and path == "vec1":
            k = F16_LONG.get(k, k)
        out.append((k, m, T))
    return out


PATH_KIND = [(p, kind) for p, v in PATHS.items() for kind in v[0]]


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def decode(kind, raw, k, m, round_f16=False):
    if kind == "INT8":
        return wq.dequantize_int8(raw[:k * m], raw[k * m:].view(np.float16).reshape(-1, 2)).reshape(m, k)
    if kind == "NF4":
        return wq.dequantize_nf4(raw[:k * m // 2], raw[k * m // 2:].view(np.float16)).reshape(m, k)
    return dq.dequantize(kind, raw, k * m, round_f16=round_f16).reshape(m, k)


@functools.lru_cache(maxsize=6)
def matrix_of(kind, k, m, enc):
    raw = br.make_blocks(kind, k, m, enc, k + m)
    return raw, decode(kind, raw, k, m).astype(np.float64), br.terms_abs(kind, raw, k, m)


def inputs_of(profile, T, k, seed):
    x = br.make_inputs(profile, (T, k), seed)
    if profile == br.SPARSE and T >= 2:         # an all-zero token (both zeros) among the sparse ones
        x[0] = np.where(np.arange(k) % 3 == 0, -0.0, 0.0).astype(np.float16)
    return x


def run(ctx, mat, x, m, turbo, out_dtype=np.float32, act="none"):
    T, k = x.shape
    out = ctx.zeros([m, T, 1], out_dtype)
    mat.matmul_op(ctx.tensor(x, [k, T, 1]), out, act, turbo=turbo)
    return out.back().reshape(T, m)


def check(got, w, terms, x, what):
    xd = x.astype(np.float64)
    want = xd @ w.T
    bound = C * (np.abs(xd) @ terms.T)
    assert np.abs(want).max() < 1e30
    assert np.isfinite(got).all(), (what, "non-finite outputs", int((~np.isfinite(got)).sum()), "of", got.size)
    err = np.abs(got.astype(np.float64) - want)
    bad = err > bound
    ratio = float((err / np.where(bound > 0, bound, 1.0))[bound > 0].max()) * C if (bound > 0).any() else 0.0
    print(f"{what}: worst |err| / (terms @ |x|) = {ratio:.3e}")
    assert not bad.any(), (what, int(bad.sum()), "outside the bound; worst ratio", ratio, "max |err|", float(err.max()))
    zero_tok = ~xd.any(axis=1)
    assert np.all(got[zero_tok] == 0.0), (what, "an all-zero token must give exactly 0.0")


@pytest.mark.parametrize("profile", br.INPUTS)
@pytest.mark.parametrize("enc", br.ENCODINGS)
@pytest.mark.parametrize("path,kind", PATH_KIND)
def test_encoding_x_input(ctx, monkeypatch, path, kind, enc, profile):
    _, _, turbo, env, _ = PATHS[path]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    for k, m, T in shapes_of(path, kind):
        raw, w, terms = matrix_of(kind, k, m, enc)
        x = inputs_of(profile, T, k, k + T)
        for flags in ((wrk.MATRIX_EXACT, wrk.MATRIX_ROUND_F16) if path == "vec1" else (wrk.MATRIX_EXACT,)):
            mat = wrk.Matrix(ctx, kind, k, m, raw, flags)
            wr = w if flags == wrk.MATRIX_EXACT else decode(kind, raw, k, m, round_f16=True).astype(np.float64)
            what = f"{path} {kind} K={k} M={m} T={T} flags={flags} {enc} x {profile}"
            check(run(ctx, mat, x, m, turbo), wr, terms, x, what)
            if T == 1:                              # the one-token kernels: an all-zero input of their own
                z = np.where(np.arange(k) % 3 == 0, -0.0, 0.0).astype(np.float16).reshape(1, k)
                assert np.all(run(ctx, mat, z, m, turbo) == 0.0), (what, "all-zero input")


@pytest.mark.parametrize("enc", br.ENCODINGS)
@pytest.mark.parametrize("path,kind", PATH_KIND)
def test_f16_output_activation_epilogue(ctx, monkeypatch, path, kind, enc):
    """f16 store behind tanh (bounded, so no encoding overflows the store), `normal` inputs: one f16 ulp of the exact value plus the
    f32 bound carried through tanh (slope <= 1) plus the 2e-5 the other matmul tests grant the device tanh."""
    _, _, turbo, env, _ = PATHS[path]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    for k, m, T in shapes_of(path, kind):
        raw, w, terms = matrix_of(kind, k, m, enc)
        x = inputs_of(br.NORMAL, T, k, k + T + 1)
        mat = wrk.Matrix(ctx, kind, k, m, raw)
        got = run(ctx, mat, x, m, turbo, np.float16, "tanh").astype(np.float64)
        xd = x.astype(np.float64)
        want = np.tanh(xd @ w.T)
        tol = np.maximum(np.abs(want), 2.0 ** -14) * 2.0 ** -10 + C * (np.abs(xd) @ terms.T) + 2e-5
        assert np.isfinite(got).all()
        assert np.all(np.abs(got - want) <= tol), (path, kind, k, m, T, enc, float(np.abs(got - want).max()))


FLIP_CASES = [(p, kind) for p, kind in PATH_KIND if kind in ("Q6_K", "Q8_0")]
# Where the two sign conventions must give the same BITS: the kernels that multiply d * sc (a sign-symmetric f32 product) into codes taken
# as they are -- Q6_K on the matvec kernels.  The others are not sign-symmetric by construction, read off the source:
#   * Q8_0 on the matvec kernels decodes u = code + 128 and subtracts 128 * sum(x) (wrk_matvec_dev.h decode_raw: off = 128): -code is
#     another u, another rounding;
#   * Q6_K on every MFMA kernel splits sc = 2 * (sc >> 1) + (sc & 1) over two MFMAs (wrk_gemm.hip gemm_body): -5 = 2 * -3 + 1, 5 = 2 * 2 + 1;
#   * Q8_0 on the MFMA kernels negates A and d exactly in the source, yet a few outputs differ in the last bit on `normal` inputs only
#     (first run on MI355X: ks18, ks28, ks44, tile2): the matrix core's 32-term f32 accumulation is not sign-symmetric.
# Those paths are held to the bound for both encodings instead, which bounds their difference by 2 * C * (terms @ |x|).
BIT_IDENTICAL = {("vec1", "Q6_K"), ("vecT", "Q6_K")}


@pytest.mark.parametrize("profile", [br.NORMAL, br.LARGE_SAME_SIGN, br.TINY])
@pytest.mark.parametrize("path,kind", FLIP_CASES)
def test_sign_flipped_encoding(ctx, monkeypatch, path, kind, profile):
    """Q6_K with d and every scale negated, Q8_0 with d and every code negated: the same weights, (-d) * (-sc) is the same f32 product.
    Bit-identical outputs where the kernel is sign-symmetric (BIT_IDENTICAL; an output that is zero may be either zero), within the bound
    for both encodings everywhere."""
    _, _, turbo, env, _ = PATHS[path]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    for k, m, T in shapes_of(path, kind):
        a = br.flippable(kind, br.make_blocks(kind, k, m, br.UNIFORM_BYTES, 17), k, m)
        b = br.flip(kind, a, k, m)
        x = inputs_of(profile, T, k, 3)
        terms = br.terms_abs(kind, a, k, m)
        for flags in ((wrk.MATRIX_EXACT, wrk.MATRIX_ROUND_F16) if path == "vec1" else (wrk.MATRIX_EXACT,)):
            ga = run(ctx, wrk.Matrix(ctx, kind, k, m, a, flags), x, m, turbo)
            gb = run(ctx, wrk.Matrix(ctx, kind, k, m, b, flags), x, m, turbo)
            w = decode(kind, a, k, m, round_f16=flags == wrk.MATRIX_ROUND_F16).astype(np.float64)
            what = f"{path} {kind} K={k} M={m} T={T} flags={flags} {profile}"
            check(ga, w, terms, x, what + " (as generated)")
            check(gb, w, terms, x, what + " (sign-flipped)")
            same = (ga.view(np.uint32) == gb.view(np.uint32)) | ((ga == 0) & (gb == 0))
            print(f"{what}: {int((~same).sum())} of {same.size} outputs differ between the sign conventions, max |diff| {float(np.abs(ga - gb).max()):.3e}")
            if (path, kind) in BIT_IDENTICAL:
                assert same.all(), (what, int((~same).sum()), float(np.abs(ga - gb).max()))


# ------------------------------------------------------------------------------------------------ model level
Q6_MIX = {"time_mix_value": "Q6_K", "channel_mix_value": "Q6_K"}


def test_model_with_sign_flipped_q6k_tensors(ctx, monkeypatch):
    """Signed Q6_K scales in the fused layer launches, the K-sliced GEMM (WRK_GEMM_KS=2; wrk_op_matmul passes no partial buffer, so the op
    cannot reach it), a prefill chunk and the head's arg-max epilogue: a synthetic model whose Q6_K tensors (attention value, ffn value,
    head) are re-encoded with d and every scale negated.
    One sequence decodes on the matvec kernels, which are sign-symmetric (BIT_IDENTICAL above): logits, greedy tokens and state have the bits
    of the unflipped model.  The batch and the chunk run on MFMA kernels, which split sc = 2 * (sc >> 1) + (sc & 1) and are not: they are
    held to the oracle layer by layer at test_gpu_layer_parity.py's own bars (the oracle decodes both encodings to the same weights)."""
    import test_gpu_layer_parity as lp
    from oracle import synth
    cfg = synth.CONFIGS["small"]
    outs = []
    for hook in (None, br.flip_tensor):
        data = synth.make_v7_gguf(cfg, 42, mat_override=Q6_MIX, reencode=hook)
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=1, weights=wrk.WEIGHTS_INLINE)
        logits = []
        for t in synth.tokens(5, "flip", 6, cfg.num_vocab):
            logits.append(rt.infer(wrk.RnnInput([[t]], 32), mode=1)[0].copy())
        tok, _ = rt.generate_greedy([int(logits[-1][0].argmax())], 6, mode=1)
        outs.append((data, np.stack(logits), tok.copy(), rt.state_back(0).copy()))
        rt.close()
    (da, la, ta, sa), (db, lb, tb, sb) = outs
    assert da != db and len(da) == len(db)                       # the hook really rewrote tensors
    assert np.isfinite(la).all()
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)) and np.array_equal(ta, tb) and np.array_equal(sa.view(np.uint32), sb.view(np.uint32))
    kw = {"mat_override": Q6_MIX, "reencode": br.flip_tensor}
    lp.run_case(ctx, "small", wrk.WEIGHTS_INLINE, kw, 1, [1], 3)                 # decode, layer by layer against the oracle
    lp.run_case(ctx, "small", wrk.WEIGHTS_INLINE, kw, 1, [70], 2)                # one prefill chunk: tile GEMMs
    monkeypatch.setenv("WRK_GEMM_KS", "2")
    lp.run_case(ctx, "small", wrk.WEIGHTS_INLINE, kw, 1, [1] * 18, 2)            # every matrix on the K-sliced kernel
