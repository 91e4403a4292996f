"""The on-device Q4_K quantiser (wrk_matrix_quantize(WRK_MAT_Q4_K)) against an f64 statement of its rule.  DESIGN.md 4.11 has the measured
error ratios, MARGIN's derivation from them (twice the largest deviation seen on either side, 1.97e-3) and the model's logit distance."""
import numpy as np
import pytest

import wrk
from oracle import dequant, quantize, synth

pytestmark = pytest.mark.gpu
MARGIN = 4e-3


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def search(x):
    """f64 [n, 32] -> (scale, offset, weights) per sub-block: the candidate search of the rule"""
    w = np.sqrt((x * x).mean(1, keepdims=True)) + np.abs(x)
    mn, mx, sw, sx = np.minimum(x.min(1), 0)[:, None], x.max(1)[:, None], w.sum(1), (w * x).sum(1)
    rng, flat = np.where(mx == mn, 1.0, mx - mn), (mx == mn)[:, 0]
    err = lambda s, m, L: (w * (s[:, None] * L + m[:, None] - x) ** 2).sum(1)
    scale, low = rng[:, 0] / 15, mn[:, 0]
    best = err(scale, low, np.clip(np.rint(15 / rng * (x - mn)), 0, 15))
    for i in range(21):
        L = np.clip(np.rint((-1 + 0.1 * i + 15) / rng * (x - mn)), 0, 15)
        sl, sl2, sxl = (w * L).sum(1), (w * L * L).sum(1), (w * L * x).sum(1)
        D = sw * sl2 - sl * sl
        ts, tm = (sw * sxl - sx * sl) / np.where(D > 0, D, 1), (sl2 * sx - sl * sxl) / np.where(D > 0, D, 1)
        ts, tm = np.where(tm > 0, sxl / np.where(sl2 > 0, sl2, 1), ts), np.where(tm > 0, 0.0, tm)
        e = err(ts, tm, L)
        take = (D > 0) & (e < best)
        scale, low, best = np.where(take, ts, scale), np.where(take, tm, low), np.where(take, e, best)
    return np.where(flat, 0.0, scale), 0.0 - np.where(flat, mn[:, 0], low), w


def final_codes(x32, d, dmin, sc, m):       # f32 [nb, 8, 32] and a stored header -> the codes, in f32
    step, off = ((a.astype(np.float32)[:, None] * b.astype(np.float32))[:, :, None] for a, b in ((d, sc), (dmin, m)))
    return np.where(step != 0, np.clip(np.rint((x32 + off) / np.where(step != 0, step, 1)), 0, 15), 0).astype(np.uint8)


def reference(w16):
    """f16 [m, k] -> (ggml's 144-byte blocks by the rule in f64, the codes in f32 from the stored header; the rule's weights)"""
    def grid(v):
        top = v.max(1, keepdims=True)
        return (top[:, 0] / 63).astype(np.float16), np.where(top > 0, np.minimum(63, np.rint(63 * v / np.where(top > 0, top, 1))), 0).astype(np.uint8)
    scale, off, w = search(w16.astype(np.float64).reshape(-1, 32))
    (d, sc), (dmin, m) = grid(scale.reshape(-1, 8)), grid(off.reshape(-1, 8))
    q = final_codes(w16.astype(np.float32).reshape(-1, 8, 32), d, dmin, sc, m).reshape(-1, 4, 2, 32)
    out = np.empty((len(d), 144), np.uint8)
    out[:, :4] = np.stack([d, dmin], 1).astype("<f2").view(np.uint8)
    out[:, 4:16], out[:, 16:] = quantize.pack_scale_min_k4(sc, m), (q[:, :, 0] | (q[:, :, 1] << 4)).reshape(-1, 128)
    return out.reshape(-1), w


@pytest.mark.parametrize("k,m", [(256, 1), (512, 5), (2048, 24)])   # one super-block | ragged against a 4-wave workgroup | a model-like row
@pytest.mark.parametrize("case", ["gauss", "zeros", "constant", "positive", "negative", "max", "subnormal", "zero sub-block"])
def test_blocks_follow_their_header_and_the_search(ctx, k, m, case):
    w = (np.random.default_rng(k + m).standard_normal((m, k)) / np.sqrt(k)).astype(np.float16)
    g, i = np.random.default_rng(7).standard_normal(256) / 16, np.arange(256)
    w[m - 1, k - 256:] = {"gauss": g, "zeros": 0 * g, "constant": 0 * g + .5, "positive": np.abs(g) + .01, "negative": -np.abs(g) - .01,
                          "max": g + 65504.0 * (i == 77), "subnormal": np.rint(g * 4096) * 2.0 ** -24, "zero sub-block": g * (i // 32 != 2)}[case]
    mat = wrk.Matrix.q4_k(wrk.Buffer(ctx, w.nbytes, w), k, m)
    raw = mat.export()
    assert raw.size == m * k // 256 * 144 and mat.stream_bytes == raw.size and (case != "zeros" or not raw[-144:].any())
    b = raw.reshape(-1, 144)
    (d, dmin), (sc, mn) = b[:, :4].copy().view("<f2").T, dequant.get_scale_min_k4(b[:, 4:16])
    assert (d >= 0).all() and (dmin >= 0).all() and not (np.signbit(d) | np.signbit(dmin)).any()
    got = np.stack([b[:, 16:].reshape(-1, 4, 32) & 15, b[:, 16:].reshape(-1, 4, 32) >> 4], axis=2).reshape(-1, 8, 32)
    assert np.count_nonzero(got != final_codes(w.astype(np.float32).reshape(-1, 8, 32), d, dmin, sc, mn)) == 0
    x, outs = ctx.tensor(np.random.default_rng(1).standard_normal((1, k)).astype(np.float16), [k, 1, 1]), []
    for mt in (mat, wrk.Matrix(ctx, "Q4_K", k, m, raw)):        # the export, created again, is the same matrix
        outs.append(ctx.zeros([m, 1, 1], np.float32))
        mt.matmul_op(x, outs[-1])
    assert np.array_equal(outs[0].back().view(np.uint32), outs[1].back().view(np.uint32))
    if case == "gauss":         # quality, on Gaussian rows: E = sum w (deq - x)^2 against the f64 search and against min/max
        x64, (ref, wt) = w.astype(np.float64).reshape(-1, 32), reference(w)
        E = lambda r: float((wt * (dequant.dequantize_q4_k(r, w.size, round_f16=False).reshape(-1, 32) - x64) ** 2).sum())
        e_gpu, e_ref, e_minmax = E(raw), E(ref), E(quantize.quantize_q4_k(w))
        print(f"k {k} m {m}: E_gpu / E_ref = {e_gpu / e_ref:.6f}, E_minmax / E_ref = {e_minmax / e_ref:.4f}")
        assert e_ref * (1 + MARGIN) < e_minmax          # the inputs tell the two quantisers apart by more than the margin
        assert e_gpu <= e_ref * (1 + MARGIN) and e_gpu < e_minmax


def test_f16_model_loads_as_q4_k_and_runs_on_the_engine(ctx, monkeypatch):
    cfg = synth.CONFIGS["tiny"]             # the smallest shape tests/test_gpu_engine.py builds an engine for
    mats = {name: dims[0] for name, dims, kind, _ in synth.v7_tensor_plan(cfg, 42) if kind == "mat"}
    def dequantised(name, tn, raw):         # the f16 twin: every big matrix is what its quantised blocks dequantise to, rounded to f16
        if name not in mats:
            return raw
        blocks = wrk.Matrix.q4_k(wrk.Buffer(ctx, raw.nbytes, raw), mats[name], raw.size // 2 // mats[name]).export()
        return dequant.dequantize_q4_k(blocks, raw.size // 2).astype(np.float16).view(np.uint8)
    data, twin = synth.make_v7_gguf(cfg, 42, mat="F16"), synth.make_v7_gguf(cfg, 42, mat="F16", reencode=dequantised)
    monkeypatch.setenv("WRK_ENGINE", "1")
    q, f = wrk.Runtime(ctx, wrk.GgufReader(data), quant={l: "q4_k" for l in range(cfg.num_layer)}), wrk.Runtime(ctx, wrk.GgufReader(twin))
    assert q.engine_status()[0], q.engine_status()[1]
    inp = lambda: wrk.RnnInput([synth.tokens(11, "prompt", 19, cfg.num_vocab)], 32)
    diff = np.abs(q.infer(inp(), mode=1)[0] - f.infer(inp(), mode=1)[0])
    print(f"q4_k against its f16 twin: max {diff.max():.3e}, mean {diff.mean():.3e}")
    assert diff.max() <= 1e-2 and diff.mean() <= 1.5e-3      # tests/test_gpu_quant_model.py's bars for NF4
    state = q.state_back(0)
    with_engine = q.generate_greedy([5], 8, mode=1)[0].tolist()
    monkeypatch.setenv("WRK_ENGINE", "0")
    q.state_load(state, 0)
    assert q.generate_greedy([5], 8, mode=1)[0].tolist() == with_engine
    q.close(), f.close()


def test_refusals(ctx):
    buf = wrk.Buffer(ctx, 256 * 8 * 2, np.zeros(256 * 8, np.float16))
    for k, levels in ((128, None), (256, np.zeros(16))):
        with pytest.raises(wrk.WrkError, match="WRK_E_ARG"):
            wrk.Matrix._quant("Q4_K", buf, k, 8, levels)
    with pytest.raises(wrk.WrkError):
        wrk.Runtime(ctx, wrk.GgufReader(synth.make_v7_gguf(synth.CONFIGS["tiny"], 7)), quant={0: 9})
