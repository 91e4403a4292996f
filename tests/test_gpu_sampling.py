"""On-device nucleus sampling (web-rwkv-gguf_amd/csrc/wrk_sample.hip; examples/chat.rs:150-190 `Sampler::sample`) against the f64
restatement in tests/sampling_ref.py, through `Context.sample_logits` and the decode loops' `Runtime.generate_sample`."""
import numpy as np
import pytest

import wrk
import sampling_ref as S
from oracle import synth
from oracle.rnn import stack_cursors

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def rows_for(V):
    """(name, logits, [(T, P)]) of the kernel test."""
    rng = np.random.default_rng(V)
    Ts = (0.1, 0.5, 1.0, 2.0)
    if V <= 1000:
        grid = [(T, P) for T in Ts for P in (0.05, 0.33, 0.71, 0.9, 1.0)]
        flat = rng.normal(0.0, 0.5, V)
        peaked = rng.normal(0.0, 3.0, V); peaked[rng.integers(V)] += 12.0
        masked = rng.normal(0.0, 2.0, V); masked[rng.random(V) < 0.5] = -np.inf; masked[rng.integers(V)] = 1.0
        dup = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0
        return [("flat", flat, grid), ("peaked", peaked, grid), ("masked", masked, grid), ("dup", dup, grid)]
    head = rng.choice(V, 24, replace=False)
    grid = [(T, P) for T in Ts for P in (0.05, 0.3, 0.7, 0.95)] + [(T, 1.0) for T in (0.1, 0.5)]
    plateau = rng.normal(0.0, 0.3, V); plateau[rng.choice(V, 200, replace=False)] += 12.0   # a flat head on a flat floor
    peaked = rng.normal(0.0, 2.0, V); peaked[head] += rng.normal(14.0, 1.0, head.size)
    masked = peaked.copy(); masked[rng.random(V) < 0.5] = -np.inf; masked[head] = peaked[head]
    dup = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0; dup[head] = np.round(rng.normal(14.0, 1.0, head.size))
    return [("plateau", plateau, grid), ("peaked", peaked, grid), ("masked", masked, grid), ("dup", dup, grid)]


@pytest.mark.parametrize("V", [1, 50, 1000, 65529, 65536])
def test_kernel_matches_the_restatement(ctx, V):
    rows, par = [], []
    for _, l, grid in rows_for(V):
        l32 = l.astype(np.float32)
        for T, P in grid:
            for seed in (1, 7):
                rows.append(l32)
                par.append((T, P, seed + len(rows)))
    x = np.stack(rows)
    T = np.array([p[0] for p in par], np.float32)
    P = np.array([p[1] for p in par], np.float32)
    seed = np.array([p[2] for p in par], np.uint32)
    step = 5
    got = ctx.sample_logits(x, T, P, seed, step=step)
    clear = 0
    for i in range(len(rows)):
        args = (x[i].astype(np.float64), float(T[i]), float(P[i]), int(seed[i]), step)
        if S.ambiguous(*args):
            continue
        clear += 1
        want = S.sample(*args)
        assert got[i] == want, (i, par[i], int(got[i]), want)
    assert clear >= 0.95 * len(rows), (clear, len(rows))
    assert (got < V).all()


def test_greedy_parameters_are_argmax_rows(ctx):
    data = synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=4)
    toks = synth.tokens(3, "greedy", 4, rt.info.num_vocab)
    logits, am = rt.infer_raw(toks, stack_cursors([1, 1, 1, 1]), [0, 1, 2, 3], mode=0, want_argmax=True)   # argmax_rows
    for T, P in ((0.0, 0.9), (1.0, 0.0), (0.0, 0.0)):
        assert np.array_equal(ctx.sample_logits(logits, T, P, seed=[1, 2, 3, 4]), am)
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (6, 70000)).astype(np.float32)
    x[1, 5] = x[1, 9] = 50.0                             # tie: the first index
    x[2, :] = -np.inf                                    # nothing above -3e38: 0
    want = [int(np.argmax(r)) if np.isfinite(r).any() else 0 for r in x]
    assert ctx.sample_logits(x, 0.0, 0.5).tolist() == want
    rt.close()


@pytest.mark.parametrize("cfg,B,mode", [("tiny", 1, 0), ("small", 1, 1), ("tiny", 4, 1), ("tiny", 4, 0)])
def test_generate_sample_top_p_zero_is_generate_greedy(ctx, cfg, B, mode):
    data = synth.make_v7_gguf(synth.CONFIGS[cfg], 42)
    first = [(5 + 61 * b) % synth.CONFIGS[cfg].num_vocab for b in range(B)]
    a = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    g, _ = a.generate_greedy(first, 12, mode=mode)
    a.close()
    b = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    s, _ = b.generate_sample(first, 12, temperature=1.0, top_p=0.0, mode=mode)
    b.close()
    assert np.array_equal(g, s)


def test_v6_generate_sample_top_p_zero_is_generate_greedy(ctx):
    data = synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42)
    for mode in (0, 1):
        a = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
        g, _ = a.generate_greedy([3, 400], 8, mode=mode)
        a.close()
        b = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
        s, _ = b.generate_sample([3, 400], 8, temperature=0.8, top_p=0.0, mode=mode)
        b.close()
        assert np.array_equal(g, s)


def chi2_sf(x, k):
    """Upper tail of chi-square with k degrees of freedom (Wilson-Hilferty)."""
    from math import erfc, sqrt
    z = ((x / k) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * k))) / sqrt(2.0 / (9.0 * k))
    return 0.5 * erfc(z / sqrt(2.0))


@pytest.mark.parametrize("T,P", [(1.0, 0.9), (0.6, 0.7), (1.8, 1.0)])
def test_draws_follow_the_tempered_nucleus(ctx, T, P):
    rng = np.random.default_rng(11)
    l = rng.normal(0, 1.5, 64).astype(np.float32)
    n = 16384
    got = ctx.sample_logits(np.tile(l, (n, 1)), T, P, seed=np.arange(n, dtype=np.uint32), step=3)
    toks, w, _ = S.nucleus(l.astype(np.float64), T, P)
    outside = np.setdiff1d(np.arange(64), toks)
    assert not np.isin(got, outside).any()
    counts = np.bincount(got, minlength=64)[toks]
    expect = w * n
    stat = float(((counts - expect) ** 2 / expect).sum())
    assert chi2_sf(stat, max(len(toks) - 1, 1)) > 1e-6, stat


def test_model_level_draws_match_the_restatement(ctx):
    data = synth.make_v7_gguf(synth.CONFIGS["small"], 42)
    B, k = 3, 10
    T, P, seed = [0.7, 1.0, 1.4], [0.9, 0.6, 1.0], [11, 12, 13]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    cur = [7, 100, 900]
    checked = 0
    for step in range(k):       # one-step calls: the draw at t = 0 on the logits the call returns
        t, _, last = rt.generate_sample(cur, 1, temperature=T, top_p=P, seed=seed, want_logits=True)
        for b in range(B):
            args = (last[b].astype(np.float64), T[b], P[b], seed[b], 0)
            if not S.ambiguous(*args):
                assert int(t[0, b]) == S.sample(*args), (step, b)
                checked += 1
        cur = t[0].tolist()
    assert checked >= B * k // 2     # the small model's logits are flat (V = 1000): about one step in five sits near a boundary
    rt.close()
    # one k-step call, replayed token by token through wrk_v7_infer's logits
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    toks, _ = rt.generate_sample([7, 100, 900], k, temperature=T, top_p=P, seed=seed)
    rt.close()
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    cur = [7, 100, 900]
    live = [True] * B
    for step in range(k):
        logits = rt.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=1)
        for b in range(B):
            args = (logits[b].astype(np.float64), T[b], P[b], seed[b], step)
            if live[b] and S.ambiguous(*args):
                live[b] = False     # the two runs may part here; later steps of this sequence are not comparable
            if live[b]:
                assert int(toks[step, b]) == S.sample(*args), (step, b)
        cur = toks[step].tolist()
    rt.close()


def test_determinism_and_groups(ctx):
    data = synth.make_v7_gguf(synth.CONFIGS["small"], 42)
    B = 4
    first = [3, 77, 200, 411]
    kw = dict(temperature=[0.9, 1.1, 1.0, 0.5], top_p=[0.95, 0.8, 1.0, 0.9])
    runs = []
    for _ in range(2):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        runs.append(rt.generate_sample(first, 16, **kw)[0])
        rt.close()
    assert np.array_equal(runs[0], runs[1])
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    grouped, _ = rt.generate_sample(first, 16, groups=2, **kw)
    rt.close()
    for b0, b1 in ((0, 2), (2, 4)):
        alone = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=b1 - b0)
        t, _ = alone.generate_sample(first[b0:b1], 16, temperature=kw["temperature"][b0:b1], top_p=kw["top_p"][b0:b1],
                                     seed=list(range(b0, b1)))
        alone.close()
        assert np.array_equal(grouped[:, b0:b1], t)


@pytest.mark.parametrize("B,mode", [(1, 1), (2, 1), (2, 0)])
def test_parameters_are_not_baked_into_the_step_program(ctx, B, mode):
    data = synth.make_v7_gguf(synth.CONFIGS["small"], 42)
    first = [9, 500][:B]
    a = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    greedy_before, _ = a.generate_greedy(first, 8, mode=mode)
    a.close()
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    rt.generate_sample(first, 8, temperature=0.7, top_p=0.8, seed=1, mode=mode)
    for b in range(B):
        rt.state_load(np.zeros_like(rt.state_back(b)), b)
    second, _ = rt.generate_sample(first, 8, temperature=1.3, top_p=0.95, seed=2, mode=mode)
    for b in range(B):
        rt.state_load(np.zeros_like(rt.state_back(b)), b)
    greedy_after, _ = rt.generate_greedy(first, 8, mode=mode)
    rt.close()
    fresh = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    want, _ = fresh.generate_sample(first, 8, temperature=1.3, top_p=0.95, seed=2, mode=mode)
    fresh.close()
    assert np.array_equal(second, want)
    assert np.array_equal(greedy_after, greedy_before)


def test_eager_path_equals_the_replayed_program(ctx, monkeypatch):
    data = synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)
    out = []
    for eager in ("0", "1"):
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
        out.append(rt.generate_sample([4, 40], 10, temperature=1.0, top_p=0.9)[0])
        rt.close()
    assert np.array_equal(out[0], out[1])


def test_argument_errors_leave_the_model_usable(ctx):
    data = synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
    V = rt.info.num_vocab
    x = np.zeros((2, 16), np.float32)
    for T, P in ((np.nan, 0.5), (-1.0, 0.5), (1.0, np.nan), (1.0, -0.1)):
        with pytest.raises(wrk.WrkError) as e:
            ctx.sample_logits(x, T, P)
        assert e.value.code == wrk.E_ARG
        with pytest.raises(wrk.WrkError) as e:
            rt.generate_sample([1, 2], 3, temperature=T, top_p=P)
        assert e.value.code == wrk.E_ARG
    with pytest.raises(wrk.WrkError):
        rt.generate_sample([1, V], 3)                   # first token out of vocab
    ft = np.array([1, 2], np.uint32)
    f = np.ones(2, np.float32)
    sd = np.zeros(2, np.uint32)
    out = np.zeros((3, 2), np.uint32)
    P_ = wrk._ptr
    for args in ((None, P_(f, wrk._f32p), P_(sd, wrk._u32p)), (P_(f, wrk._f32p), None, P_(sd, wrk._u32p)), (P_(f, wrk._f32p), P_(f, wrk._f32p), None)):
        rc = wrk.hip.wrk_v7_generate_sample(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, *args, P_(out, wrk._u32p), None, None, 1)
        assert rc == wrk.E_ARG
    buf = ctx.buffer(x)
    f3, s3 = np.ones(3, np.float32), np.zeros(3, np.uint32)
    assert wrk.hip.wrk_sample_logits(ctx.h, buf.h, 16, 16, 2, None, P_(f, wrk._f32p), P_(sd, wrk._u32p), 0, P_(sd, wrk._u32p)) == wrk.E_ARG
    assert wrk.hip.wrk_sample_logits(ctx.h, buf.h, 16, 16, 3, P_(f3, wrk._f32p), P_(f3, wrk._f32p), P_(s3, wrk._u32p), 0,
                                     P_(s3, wrk._u32p)) == wrk.E_ARG       # 3 rows exceed the buffer
    # still usable: the greedy loop from a zero state equals a fresh runtime's, and a sampled call runs
    for b in range(2):
        rt.state_load(np.zeros_like(rt.state_back(b)), b)
    g, _ = rt.generate_greedy([1, 2], 4)
    fresh = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
    assert np.array_equal(g, fresh.generate_greedy([1, 2], 4)[0])
    fresh.close()
    t, _ = rt.generate_sample([1, 2], 4, temperature=1.0, top_p=0.9)
    assert t.shape == (4, 2) and (t < V).all()
    rt.close()
