"""RWKV-6 path: V6-only ops and whole-model parity against oracle/rwkv6.py.
PARITY UNPINNED against the real reference (no V6 test or fixture exists there)."""
import numpy as np
import pytest

import wrk
from oracle import gguf as ogguf
from oracle import rwkv6 as O6
from oracle import rwkv7 as O
from oracle import synth
from oracle.rnn import stack_cursors

pytestmark = pytest.mark.gpu
LOGIT_TOL, LOGIT_MEAN_TOL = 1e-2, 1.5e-3


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def close16(got, want, ulps=1.0):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    tol = ulps * np.maximum(np.abs(want), 2.0 ** -14) * 2.0 ** -10 + 1e-6
    assert np.all(np.abs(got - want) <= tol), np.abs(got - want).max()


def test_token_shift_per_token_factors_and_transpose(ctx):
    """token_shift with a [C, T, 5] factor tensor (v6.rs:804-812) and transpose [R,5,T] -> [R,T,5] (:793)."""
    C, lens = 256, [3, 2]
    T, B = sum(lens), 2
    r = np.random.default_rng(3)
    x = h16(r.standard_normal((T, C)))
    fac = h16(r.random((5, T, C)))
    state = r.standard_normal((B, 66, C)).astype(np.float32)
    out = ctx.zeros([C, T, 5])
    wrk.TensorOp.token_shift(ctx.buffer(np.array(stack_cursors(lens), np.uint32)), ctx.tensor(fac), ctx.tensor(state).view(None, 0),
                             ctx.tensor(x, [C, T, 1]), out, True)
    prev = np.empty((T, C), np.float32)
    prev[1:] = x[:-1]
    prev[0], prev[3] = state[0, 0], state[1, 0]
    want = O.r16(O.mix(x.astype(np.float32)[None], prev[None], fac.astype(np.float32)))
    close16(out.back().reshape(5, T, C), want)
    a = h16(r.standard_normal((T, 5, 32)))
    t = ctx.zeros([32, T, 5])
    wrk.TensorOp.transpose(ctx.tensor(a), t)
    assert np.array_equal(t.back().reshape(5, T, 32), a.transpose(1, 0, 2))


@pytest.mark.parametrize("wave,octs", [("0", "0"), ("0", "1"), ("1", "0")])
@pytest.mark.parametrize("lens,H", [([1], 4), ([4, 0, 3], 4), ([7, 1, 13, 4], 2), ([70, 66], 1)])
def test_time_mix_v6(ctx, lens, H, wave, octs, monkeypatch):
    # the chunk kernels of the dense layout (round 3): four | eight threads per state column (the latter with a head's columns over several
    # workgroups) | one wave per head: tails of the 3- / 4-token prefetch rings, an empty batch, more than 64 stacked tokens
    monkeypatch.setenv("WRK_WKV_WAVE", wave)
    monkeypatch.setenv("WRK_WKV_OCT", octs)
    S, B = 64, len(lens)
    D, T = H * S, sum(lens)
    r_ = np.random.default_rng(T)
    k, v, rr = (r_.standard_normal((T, D)).astype(np.float32) * s for s in (0.5, 1.0, 1.0))
    w = np.exp(-np.exp(r_.uniform(-3, 0.5, (T, D)))).astype(np.float32)
    u = (0.3 * r_.standard_normal(D)).astype(np.float32)
    xln = h16(r_.standard_normal((T, D)))
    state = (0.3 * r_.standard_normal((B, S + 2, D))).astype(np.float32)
    st, x = ctx.tensor(state), ctx.tensor(xln, [S, H, T])
    f = lambda a: ctx.tensor(a, [S, H, T])
    wrk.TensorOp.time_mix_v6(ctx.buffer(np.array(stack_cursors(lens), np.uint32)), f(w), ctx.buffer(u), st.view(None, (0, S + 1)), f(k), f(v), f(rr), x)
    cur = stack_cursors(lens)
    want_y, stw = np.empty((T, D), np.float32), state.copy()
    for t in range(T):
        b, start, n = cur[t] & 0xFF, (cur[t] >> 8) & 0xFFFF, cur[t] >> 24
        if t - start + 1 == n:
            stw[b, 0] = xln[start + n - 1]
        Sm = stw[b, 1:S + 1].reshape(S, H, S).transpose(1, 0, 2)
        kv = k[t].reshape(H, S)[:, :, None] * v[t].reshape(H, S)[:, None, :]
        want_y[t] = np.einsum("hj,hji->hi", rr[t].reshape(H, S), u.reshape(H, S)[:, :, None] * kv + Sm).reshape(D)
        stw[b, 1:S + 1] = (w[t].reshape(H, S)[:, :, None] * Sm + kv).transpose(1, 0, 2).reshape(S, D)
    np.testing.assert_allclose(st.back().reshape(B, S + 2, D), stw, rtol=1e-4, atol=1e-4)
    close16(x.back().reshape(T, D), O.r16(want_y), 2)


def test_time_mix_v6_chunk_kernels_are_bit_identical(ctx, monkeypatch):
    """four waves per head and one wave per head sum over j in the same order"""
    S, H, lens = 64, 3, [9, 0, 22]
    B, D, T = len(lens), H * S, sum(lens)
    r_ = np.random.default_rng(5)
    k, v, rr = (r_.standard_normal((T, D)).astype(np.float32) * s for s in (0.5, 1.0, 1.0))
    w = np.exp(-np.exp(r_.uniform(-3, 0.5, (T, D)))).astype(np.float32)
    u = (0.3 * r_.standard_normal(D)).astype(np.float32)
    xln = h16(r_.standard_normal((T, D)))
    state = (0.3 * r_.standard_normal((B, S + 2, D))).astype(np.float32)
    got = []
    monkeypatch.setenv("WRK_WKV_OCT", "0")          # (eight threads per column split each chain of sixteen: equal within the oracle bound only)
    for wave in ("0", "1"):
        monkeypatch.setenv("WRK_WKV_WAVE", wave)
        st, x = ctx.tensor(state), ctx.tensor(xln, [S, H, T])
        f = lambda a: ctx.tensor(a, [S, H, T])
        wrk.TensorOp.time_mix_v6(ctx.buffer(np.array(stack_cursors(lens), np.uint32)), f(w), ctx.buffer(u), st.view(None, (0, S + 1)), f(k), f(v), f(rr), x)
        got.append((st.back().copy(), x.back().copy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1].view(np.uint16), got[1][1].view(np.uint16))


def test_channel_mix_v6(ctx):
    C, lens = 256, [2, 3]
    T = sum(lens)
    r_ = np.random.default_rng(4)
    rr, v, x = (h16(r_.standard_normal((T, C))) for _ in range(3))
    state = r_.standard_normal((2, 66, C)).astype(np.float32)
    st, xt = ctx.tensor(state), ctx.tensor(x, [C, T, 1])
    wrk.TensorOp.channel_mix(ctx.buffer(np.array(stack_cursors(lens), np.uint32)), st.view(None, 65), ctx.tensor(rr, [C, T, 1]), ctx.tensor(v, [C, T, 1]), xt)
    got = st.back().reshape(2, 66, C)
    assert np.array_equal(got[0, 65], x[1].astype(np.float32)) and np.array_equal(got[1, 65], x[4].astype(np.float32))
    close16(xt.back().reshape(T, C), O.r16(O.sigmoid(rr.astype(np.float32)) * v.astype(np.float32)), 2)


# FIXED bars per fixture (no sliding bar).  2 layers: the V7 bars.  7 layers: an f16 flip propagates through more
# layers -- the oracle against ITSELF with f64 matmul accumulation differs by 8.1e-3 max / 1.9e-3 mean on this fixture (printed below
# as a diagnostic, not used as a bar) -- so the depth-7 bars are 2.5e-2 / 5e-3.
V6_BARS = {"tiny": (1e-2, 1.5e-3), "small": (2.5e-2, 5e-3)}


@pytest.mark.parametrize("name,weights,kw", [
    ("tiny", wrk.WEIGHTS_INLINE, {}),
    ("tiny", wrk.WEIGHTS_INLINE_F16, {}),
    ("tiny", wrk.WEIGHTS_INLINE, {"mat": "Q8_0", "head": "F16"}),
    ("small", wrk.WEIGHTS_INLINE, {"mat": "Q4_K"}),          # 7 layers: rescale-by-half after layer 6 + discounted w_o / ffn.value
])
def test_v6_prefill_then_greedy_decode(ctx, name, weights, kw):
    data = synth.make_v6_gguf(synth.V6_CONFIGS[name], 42, **kw)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2, weights=weights)
    assert rt.info.version == 6
    model = O6.build_v6(ogguf.GgufReader(data), weights_f16=(weights != wrk.WEIGHTS_INLINE))
    oracle = O6.V6Runtime(model, 2, act_f16=True)
    V = rt.info.num_vocab
    p0, p1 = synth.tokens(3, "v6a", 19, V), synth.tokens(3, "v6b", 5, V)
    got = rt.infer(wrk.RnnInput([p0, p1], 32))
    want = oracle.infer_chunk([p0, p1], [18, 23])

    # Diagnostic only: the noise floor of the arithmetic itself -- the same oracle with its matmuls accumulated in f64 instead
    # of f32 (only the last bit of each f32 sum moves, but f16 stores flip and the flips propagate with depth).
    class F64Acc(O6.V6Runtime):
        def _mm(self, w, x, act="none", f32_out=False):
            y = O.ACT[act]((x.astype(np.float64) @ w.T.astype(np.float64)).astype(np.float32))
            return y if f32_out else self.rnd(y)
    self_d = np.abs(F64Acc(model, 2, act_f16=True).infer_chunk([p0, p1], [18, 23]) - want)
    print(f"v6 {name}: oracle f32-vs-f64 accumulation moves the logits by max {self_d.max():.2e} / mean {self_d.mean():.2e}")
    tol_max, tol_mean = V6_BARS[name]
    toks = []
    for b in range(2):
        d = np.abs(got[b][0] - want[b])
        assert d.max() <= tol_max and d.mean() <= tol_mean, (b, d.max(), d.mean(), tol_max, tol_mean)
        toks.append(int(want[b].argmax()))
        assert int(got[b][0].argmax()) == toks[b]
    gen, ms = rt.generate_greedy(toks, 8)
    for step in range(8):
        ol = oracle.infer_chunk([[toks[0]], [toks[1]]], [0, 1])
        toks = [int(ol[0].argmax()), int(ol[1].argmax())]
        assert gen[step].tolist() == toks
    for b in range(2):
        d = np.abs(rt.state_back(b) - oracle.state[:, b])
        assert d.max() <= 3e-2 * max(1.0, float(np.abs(oracle.state).max())) and d.mean() <= max(1e-3, tol_mean)
    rt.close()


def test_v6_generate_rejects_a_state_of_another_model(ctx):
    """Generation checks that the state belongs to the model, as wrk_v6_infer does: the state of a different-sized model is
    E_ARG, not a walk over someone else's rows.  (The small model's state is the larger one.)"""
    tiny = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42)), num_batch=1, weights=wrk.WEIGHTS_INLINE)
    small = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v6_gguf(synth.V6_CONFIGS["small"], 42)), num_batch=1, weights=wrk.WEIGHTS_INLINE)
    cs, ct = synth.V6_CONFIGS["small"], synth.V6_CONFIGS["tiny"]
    assert (cs.num_layer, cs.num_emb) != (ct.num_layer, ct.num_emb) and cs.num_layer >= ct.num_layer and cs.num_emb >= ct.num_emb
    first, out = np.array([1], np.uint32), np.zeros((4, 1), np.uint32)
    rc = wrk.hip.wrk_v6_generate_greedy(ctx.h, tiny.model6, small.state, wrk._ptr(first, wrk._u32p), 1, 4, wrk._ptr(out, wrk._u32p), None, None, 1)
    assert rc == wrk.E_ARG
    tiny.close(); small.close()


def test_v6_decode_loops_ignore_the_lane_bits(ctx):
    """RWKV-6 runs one lane: bits 8-15 of the mode word (RWKV-7's number of concurrent pipelines) change nothing in generate_greedy and
    generate_stop -- same fused step, same tokens, last logits and state slots, bit for bit, as mode 1 from the same zeroed state.  The
    Python wrapper masks the bits for RWKV-6 (Runtime._mode), so the calls go to the C entry points."""
    import ctypes as C
    B, steps = 2, 4
    rt = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42)), num_batch=B, weights=wrk.WEIGHTS_INLINE)
    V = rt.info.num_vocab
    first = np.array([7, 100], np.uint32)
    zero = np.zeros_like(rt.state_back(0))

    def run(entry, mode):
        for b in range(B):
            rt.state_load(zero, b)
        tok, logits = np.zeros((steps, B), np.uint32), np.zeros((B, V), np.float32)
        head = (ctx.h, rt.model6, rt.state, wrk._ptr(first, wrk._u32p), B, steps)
        if entry == "greedy":
            rc = wrk.hip.wrk_v6_generate_greedy(*head, wrk._ptr(tok, wrk._u32p), wrk._ptr(logits, wrk._f32p), None, mode)
        else:
            opt, lens, ran = wrk.GenerateOptions(), np.zeros(B, np.uint32), C.c_uint32()
            rc = wrk.hip.wrk_v6_generate_stop(*head, C.byref(opt), wrk._ptr(tok, wrk._u32p), wrk._ptr(lens, wrk._u32p),
                                              wrk._ptr(logits, wrk._f32p), C.byref(ran), None, mode)
            assert lens.tolist() == [steps] * B and ran.value == steps
        ctx.check(rc)
        return tok, logits.view(np.uint32), [rt.state_back(b).view(np.uint32) for b in range(B)]

    try:
        for entry in ("greedy", "stop"):
            want, got = run(entry, 1), run(entry, 1 | 2 << 8)
            assert np.abs(want[2][0]).max() > 0
            assert np.array_equal(got[0], want[0]), entry
            assert np.array_equal(got[1], want[1]), entry
            for b in range(B):
                assert np.array_equal(got[2][b], want[2][b]), (entry, b)
    finally:
        rt.close()


@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("mat", ["Q5_K", "Q8_0"])
def test_v6_fused_decode_matches_op_by_op_and_oracle(ctx, B, mat):
    """The 7-launch fused decode (mode 1: LN prologues, v6_mix / v6_head kernels, gated epilogue; B = 1 register-input
    matvecs, B = 3 multi-token matvec, B = 5 MFMA) against the one-kernel-per-op path (mode 0) and the oracle."""
    cfg = synth.V6_CONFIGS["small"]
    data = synth.make_v6_gguf(cfg, 11, mat=mat)
    first = [(7 + 31 * b) % (cfg.num_vocab - 1) for b in range(B)]
    rt1 = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B, weights=wrk.WEIGHTS_INLINE)
    rt0 = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B, weights=wrk.WEIGHTS_INLINE)
    t1, _, l1 = rt1.generate_greedy(first, 10, mode=1, want_logits=True)
    t0, _, l0 = rt0.generate_greedy(first, 10, mode=0, want_logits=True)
    assert t1.tolist() == t0.tolist()
    assert np.abs(l1 - l0).max() <= 3e-2 and np.abs(l1 - l0).mean() <= 6e-3
    for b in range(B):
        d = np.abs(rt1.state_back(b) - rt0.state_back(b))
        assert d.max() <= 3e-2 * max(1.0, float(np.abs(rt0.state_back(b)).max())) and d.mean() <= 2e-3
    model = O6.build_v6(ogguf.GgufReader(data), weights_f16=False)
    oracle = O6.V6Runtime(model, B, act_f16=True)
    toks = list(first)
    for step in range(10):
        ol = oracle.infer_chunk([[t] for t in toks], list(range(B)))
        toks = [int(ol[b].argmax()) for b in range(B)]
        assert t1[step].tolist() == toks, step
    rt1.close(); rt0.close()


def test_v6_merged_prefill_launches_are_bit_identical_to_the_op_list(ctx):
    """Mode 1 runs a multi-token RWKV-6 chunk with fewer launches (blit + LN in one pass, the five LoRA ups / the five
    att projections / ffn key + receptance grouped into one MFMA launch each, W_o's add in the epilogue, both ffn shifts
    in one pass).  Same arithmetic, so above 64 stacked tokens logits and state must equal mode 0's exactly."""
    cfg = synth.V6_CONFIGS["small"]
    data = synth.make_v6_gguf(cfg, 5, mat="Q4_K")
    V = cfg.num_vocab
    p0, p1 = synth.tokens(9, "v6m-a", 70, V), synth.tokens(9, "v6m-b", 26, V)
    out = []
    for mode in (0, 1):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2, weights=wrk.WEIGHTS_INLINE)
        a = rt.infer(wrk.RnnInput([p0, p1], 96, [wrk.RNN_FULL, wrk.RNN_LAST]), mode=mode)
        b = rt.infer(wrk.RnnInput([[3] * 40, [5] * 33], 128), mode=mode)
        out.append((a + b, rt.state_back(0), rt.state_back(1)))
        rt.close()
    for x, y in zip(out[0][0], out[1][0]):
        assert np.array_equal(x, y), float(np.abs(x - y).max())
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_llama_cpp_tensor_names_run_identically(ctx):
    """BASELINE cfg 4 / 5 files come from llama.cpp's converter (time_mix_lerp_*, time_mix_decay*, ...): the same weights under those
    names must produce bit-identical logits and state (tests/test_abi_host.py checks the name resolution itself)."""
    cfg = synth.V6_CONFIGS["tiny"]
    V = cfg.num_vocab
    p = synth.tokens(21, "llama-names", 32, V)        # one 32-token chunk
    out = []
    for names in ("attn", "llama"):
        rt = wrk.Runtime(ctx, wrk.GgufReader(synth.make_v6_gguf(cfg, 42, names=names)), num_batch=1)
        a = rt.infer(wrk.RnnInput([p], 64), mode=1)[0]
        t, _, l = rt.generate_greedy([int(a[0].argmax())], 6, mode=1, want_logits=True)
        out.append((a, t, l, rt.state_back(0)))
        rt.close()
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y)
