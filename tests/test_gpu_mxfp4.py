"""MXFP4 (WRK_MAT_MXFP4, GGUF type 39) on the GPU: matvec, GEMM, quantiser, model twins, refusals.

The references are NumPy statements of the format (include/wrk_hip.h): a dequantiser, the OCP MX quantiser, and W @ x in f64.  MXFP4
weights are exact in f64 and the kernels sum exact f16 x f16 products in f32, so the matmul bar is the one tests/test_gpu_matvec.py
holds Q4_K to on the same paths: |y - y64| <= 4e-6 * sum|w||x| + 1e-6.  The model twins hold the bars of tests/test_gpu_quant_model.py.
"""
import numpy as np
import pytest

import wrk
from oracle import synth
from oracle.gguf import write_gguf

pytestmark = pytest.mark.gpu
E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def dequant(raw, k):
    """block stream (u8 e; u8 qs[16]: element j the low, element j + 16 the high nibble of qs[j]) -> f64 [m, k]"""
    b = np.asarray(raw, np.uint8).reshape(-1, 17)
    codes = np.concatenate([b[:, 1:] & 15, b[:, 1:] >> 4], axis=1)
    return (E2M1[codes] * np.exp2(b[:, :1].astype(np.float64) - 127)).reshape(-1, k)


def quant(w16):
    """f16 [m, k] -> block stream by the OCP MX rule: e = clamp(floor(log2 amax) - 2 + 127, 0, 254), nearest e2m1 value, ties to even"""
    v = w16.astype(np.float64).reshape(-1, 32)
    amax = np.abs(v).max(axis=1)
    e = np.where(amax > 0, np.clip(np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2 + 127, 0, 254), 0)
    a = np.abs(v) / np.exp2(e - 127)[:, None]
    # midpoints between neighbours; at .75, 1.75 and 3.5 the even code is the upper one, above 5 everything is 6
    code = sum(((a >= t) if t in (.75, 1.75, 3.5) else (a > t)).astype(np.uint8) for t in (.25, .75, 1.25, 1.75, 2.5, 3.5, 5.0))
    code = np.where(amax[:, None] > 0, code | (np.signbit(v).astype(np.uint8) << 3), 0).astype(np.uint8)
    out = np.empty((len(v), 17), np.uint8)
    out[:, 0], out[:, 1:] = e, code[:, :16] | (code[:, 16:] << 4)
    return out.reshape(-1)


def blocks(k, m, profile, seed):
    r = np.random.default_rng(seed)
    b = r.integers(0, 256, (k // 32 * m, 17), dtype=np.uint8)
    b[0, 1:9] = [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]          # every code is present
    b[:, 0] = r.integers(115, 131, len(b)) if profile == "typical" else r.choice([0, 1, 103, 104, 140, 141, 254], len(b))
    return b.reshape(-1)


def inputs(k, tokens, profile, dtype, seed):
    x = np.random.default_rng(seed).standard_normal((tokens, k))
    return (x * (1.0 if profile == "typical" else 2.0 ** -20)).astype(dtype)      # whole range: keeps 6 * 2^127 * sum|x| finite in f32


def run(ctx, mat, x, k, m, act="none"):
    out = ctx.zeros([m, len(x), 1], np.float32)
    mat.matmul_op(ctx.tensor(x, [k, len(x), 1]), out, act, turbo=True)
    return out.back().reshape(len(x), m)


# one block | ragged tails of the lane / wave splits | both sides of the matvec / GEMM switch | the K split over waves (8192) | two passes (16384)
SHAPES = [(32, 8, 1), (96, 24, 1), (2048, 264, 1), (4096, 8, 2), (4096, 8, 4), (256, 40, 5), (1056, 264, 33), (2048, 256, 130),
          (8192, 12, 1), (16384, 8, 3)]


# f16 inputs everywhere, f32 inputs where the matvec runs (up to 4 tokens)
@pytest.mark.parametrize("k,m,tokens,dtype", [s + (d,) for s in SHAPES for d in (np.float16, np.float32) if d == np.float16 or s[2] <= 4])
@pytest.mark.parametrize("profile", ["typical", "range"])
def test_matmul_against_f64(ctx, k, m, tokens, dtype, profile):
    raw = blocks(k, m, profile, k + m)
    mat = wrk.Matrix(ctx, "MXFP4", k, m, raw)
    assert mat.stream_bytes == m * ((k // 2 + k // 32 + 15) // 16 * 16)
    w, x = dequant(raw, k), inputs(k, tokens, profile, dtype, tokens)
    got = run(ctx, mat, x, k, m)
    want = x.astype(np.float64) @ w.T
    assert np.isfinite(want).all() and np.all(np.abs(got - want) <= 4e-6 * (np.abs(x).astype(np.float64) @ np.abs(w).T) + 1e-6), np.abs(got - want).max()


@pytest.mark.parametrize("k,m,tokens", [(2048, 264, 1), (1056, 264, 33)])
def test_scale_and_activation(ctx, k, m, tokens):
    raw = blocks(k, m, "typical", 5)
    w, x = dequant(raw, k), inputs(k, tokens, "typical", np.float16, 6)
    mat = wrk.Matrix(ctx, "MXFP4", k, m, raw)
    mat.set_scale(2.0 ** -3)
    z = (x.astype(np.float64) @ w.T) / 8
    bound = 4e-6 * (np.abs(x).astype(np.float64) @ np.abs(w).T) / 8 + 1e-6
    assert np.all(np.abs(run(ctx, mat, x, k, m) - z) <= bound)
    # |relu(z + dz)^2 - relu(z)^2| <= (2 |z| + dz) dz, and the two f32 roundings of the square: 2 * 2^-24 z^2
    assert np.all(np.abs(run(ctx, mat, x, k, m, "squared_relu") - np.maximum(z, 0) ** 2) <= (2 * np.abs(z) + bound) * bound + 2.0 ** -23 * z * z + 1e-6)


SPECIAL = {"gauss": None, "zeros": np.zeros(32), "pow2": np.r_[4.0, np.linspace(-3.9, 3.9, 31)],
           "ties": np.r_[6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, -.25, -.75, -1.25, -1.75, -2.5, -3.5, -5, np.zeros(17)] * 2.0 ** -7,
           "max": np.r_[65504.0, np.linspace(-60000, 60000, 31)], "subnormal": np.arange(32) * 2.0 ** -24 * np.r_[1, -1] .repeat(16)}


@pytest.mark.parametrize("k,m", [(32, 1), (2048, 24)])
@pytest.mark.parametrize("block", list(SPECIAL))
def test_quantiser_is_the_mx_rule_and_round_trips(ctx, k, m, block):
    w = (np.random.default_rng(k).standard_normal((m, k)) / np.sqrt(k)).astype(np.float16)
    if SPECIAL[block] is not None:
        w[m - 1, k - 32:] = SPECIAL[block].astype(np.float16)
    mat = wrk.Matrix.mxfp4(wrk.Buffer(ctx, w.nbytes, w), k, m)
    raw = mat.export()
    assert np.array_equal(raw, quant(w))
    x = inputs(k, 1, "typical", np.float16, 1)
    assert np.array_equal(run(ctx, mat, x, k, m), run(ctx, wrk.Matrix(ctx, "MXFP4", k, m, raw), x, k, m))


def twin_files(version):
    """(an F16 model, its twin whose big matrices are the dequantised MXFP4 blocks of the first -- exact in f16 for these weights)"""
    cfg, plan = (synth.CONFIGS["tiny"], synth.v7_tensor_plan) if version == 7 else (synth.V6_CONFIGS["tiny"], synth.v6_tensor_plan)
    arch = f"rwkv{version}"
    meta = [("general.architecture", "str", arch), ("general.alignment", "u32", 32), (arch + ".block_count", "u32", cfg.num_layer),
            (arch + ".embedding_length", "u32", cfg.num_emb), (arch + ".wkv.head_size", "u32", cfg.head_size)]
    if version == 7:
        meta += [(arch + ".feed_forward_length", "u32", cfg.num_hidden), (arch + ".attention.layer_norm_epsilon", "f32", 1e-5)]
    files = []
    for twin in (False, True):
        tensors = []
        for name, dims, kind, vals in plan(cfg, 3):
            tn = "F16" if kind in ("mat", "emb") else ("Q6_K" if kind == "head" else "F32")
            raw = synth.QUANTIZE[tn](vals.astype(np.float32))
            if twin and kind == "mat":
                w16 = np.asarray(raw).view(np.float16).reshape(-1, dims[0])
                deq = dequant(quant(w16), dims[0]).astype(np.float16)
                assert np.array_equal(deq.astype(np.float64), dequant(quant(w16), dims[0]))
                raw = deq.reshape(-1).view(np.asarray(raw).dtype).reshape(np.asarray(raw).shape)
            tensors.append((name, dims, tn, raw))
        files.append(write_gguf(meta, tensors))
    return files


@pytest.mark.parametrize("version,tol,mean_tol", [(7, 1e-2, 1.5e-3), (6, 3e-2, 6e-3)])     # tests/test_gpu_quant_model.py's bars
def test_model_matches_its_f16_twin(ctx, version, tol, mean_tol):
    plain, twin = twin_files(version)

    def close(a, b):
        assert np.abs(a - b).max() <= tol and np.abs(a - b).mean() <= mean_tol, (np.abs(a - b).max(), np.abs(a - b).mean())

    def mx():
        return wrk.Runtime(ctx, wrk.GgufReader(plain), num_batch=1, weights=wrk.WEIGHTS_INLINE, quant={0: "mxfp4", 1: "mxfp4"})

    V = synth.CONFIGS["tiny"].num_vocab if version == 7 else synth.V6_CONFIGS["tiny"].num_vocab
    prompt = synth.tokens(4, "prompt", 40, V)
    for mode in (0, 1):
        a, b = mx(), wrk.Runtime(ctx, wrk.GgufReader(twin), num_batch=1, weights=wrk.WEIGHTS_INLINE)
        la, lb = (r.infer(wrk.RnnInput([prompt[:14]], 32), mode=mode)[0] for r in (a, b))
        close(la, lb)
        tok = int(lb[0].argmax())
        assert a.generate_greedy([tok], 16, mode=mode)[0].tolist() == b.generate_greedy([tok], 16, mode=mode)[0].tolist()
        a.close(), b.close()
    chunk, steps = mx(), mx()
    inp, lc = wrk.RnnInput([prompt], 64), []
    while not len(lc):          # the scheduler may cut the 40 tokens into more than one prefill chunk
        lc = chunk.infer(inp, mode=1)[0]
    for t in prompt:
        ls = steps.infer(wrk.RnnInput([[t]], 32), mode=1)[0]
    close(lc, ls)
    chunk.close(), steps.close()


def test_refusals(ctx):
    for kwargs, k, code in (({}, 48, wrk.E_ARG), ({"flags": wrk.MATRIX_ROUND_F16}, 64, wrk.E_UNSUPPORTED), ({"sparse": True}, 256, wrk.E_UNSUPPORTED)):
        with pytest.raises(wrk.WrkError) as err:
            wrk.Matrix(ctx, "MXFP4", k, 8, np.zeros(k // 32 * 17 * 8, np.uint8), **kwargs)
        assert err.value.code == code
