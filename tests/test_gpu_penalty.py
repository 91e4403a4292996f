"""Repetition penalties on the device (web-rwkv-gguf_amd/csrc/wrk_penalty.hip; ChatRWKV's alpha_presence / alpha_frequency / alpha_decay /
token_ban) against the f32 restatement in tests/penalty_ref.py, through `wrk.Occurrence`, `Context.penalize_logits` and the decode
loops' `Runtime.generate_penalized`."""
import numpy as np
import pytest

import penalty_ref as R
import sampling_ref as S
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def random_slot(rng, V):
    counts = rng.uniform(0.0, 6.0, V).astype(np.float32)
    counts[rng.random(V) < 0.3] = 0.0
    flags = rng.integers(0, 4, V).astype(np.uint32)
    if V == 1:
        flags[:] = R.PRESENT
    elif (flags & R.BANNED).all():
        flags[0] = 0
    return counts, flags


def fresh(ctx, data, B):
    return wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)


def model(cfg="small", v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS[cfg], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS[cfg], 42)


def vocab(cfg="small", v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)[cfg].num_vocab


# ----------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("V", [1, 50, 1000, 65529, 65536])
def test_penalize_kernel_is_bit_exact(ctx, V, tight):
    rng = np.random.default_rng(V + (7 if tight else 0))
    B, first, n = 6, 2, 4
    stride = V if tight else V + (1 if V % 2 == 0 else 2)        # odd strides take the scalar path
    occ = wrk.Occurrence(ctx, B, V)
    slots = [random_slot(rng, V) for _ in range(B)]
    for b, (c, f) in enumerate(slots):
        occ.load(b, c, f)
    x = rng.normal(0.0, 3.0, (n, stride)).astype(np.float32)
    x[rng.random((n, stride)) < 0.05] = -np.inf
    x[rng.random((n, stride)) < 0.05] = np.nan
    ap = np.array([0.3, -0.7, 0.0, 2.5], np.float32)
    af = np.array([0.2, 0.05, -1.25, 0.0], np.float32)
    buf = ctx.buffer(x.reshape(-1))
    ctx.penalize_logits(buf, occ, ap, af, first_batch=first, num_vocab=V, row_stride=stride)
    got = buf.read(np.float32, n * stride).reshape(n, stride)
    for r in range(n):
        c, f = slots[first + r]
        want = R.penalize(x[r, :V], c, f, ap[r], af[r])
        assert np.array_equal(np.isnan(got[r, :V]), np.isnan(want)), r
        ok = ~np.isnan(want)
        assert np.array_equal(bits(got[r, :V])[ok], bits(want)[ok]), r
        assert np.array_equal(bits(got[r, V:]), bits(x[r, V:])), r         # the padding between rows is not touched
    # zero penalties and no bans: the identity, NaN and -inf included
    for b in range(B):
        occ.load(b, slots[b][0], slots[b][1] & R.PRESENT)
    y = ctx.penalize_logits(x[:, :V], occ, 0.0, 0.0, first_batch=1)
    assert np.array_equal(bits(y), bits(x[:, :V]))
    occ.close()


@pytest.mark.parametrize("decay", [1.0, 0.996, 0.0])
@pytest.mark.parametrize("V", [50, 1001, 65536])
def test_occurrence_add_is_bit_exact(ctx, V, decay):
    rng = np.random.default_rng(V)
    occ = wrk.Occurrence(ctx, 3, V)
    w = rng.uniform(0.0, 2.0, V).astype(np.float32)
    w[rng.random(V) < 0.3] = 0.0
    occ.set_weights(w)
    c0, f0 = random_slot(rng, V)
    occ.load(1, c0, f0)
    toks = rng.integers(0, V, 40).tolist()
    toks += [toks[0], toks[0], toks[3], int(np.flatnonzero(w == 0)[0])]      # repeats and a weight-0 token
    occ.add(1, toks, decay)
    c, f = occ.back(1)
    wc, wf = R.update_all(c0, f0, toks, w, decay)
    assert np.array_equal(bits(c), bits(wc))
    assert np.array_equal(f, wf)
    for b in (0, 2):                                                # the other slots are untouched
        cb, fb = occ.back(b)
        assert not cb.any() and not fb.any()
    occ.add(1, [toks[1]], decay)                                   # one token at a time: the decode loop's launch shape
    wc, wf = R.update(wc, wf, toks[1], w, decay)
    c, f = occ.back(1)
    assert np.array_equal(bits(c), bits(wc)) and np.array_equal(f, wf)
    occ.load(1)
    c, f = occ.back(1)
    assert not c.any() and not f.any()
    occ.close()


# ----------------------------------------------------------------------------------------------------------------- decode loops
CASES = [("small", 1, 1, 1, False), ("tiny", 4, 0, 1, False), ("tiny", 4, 1, 1, False), ("small", 4, 1, 2, False),
         ("tiny", 2, 0, 1, True), ("tiny", 2, 1, 1, True)]


@pytest.mark.parametrize("cfg,B,mode,groups,v6", CASES)
def test_zero_penalties_are_the_plain_sampler(ctx, cfg, B, mode, groups, v6):
    data = model(cfg, v6)
    V = vocab(cfg, v6)
    first = [(5 + 61 * b) % V for b in range(B)]
    kw = dict(temperature=[1.0, 0.8, 1.2, 0.6][:B], top_p=[0.9, 1.0, 0.7, 0.95][:B], seed=[3, 4, 5, 6][:B], mode=mode, groups=groups)
    a = fresh(ctx, data, B)
    want, _ = a.generate_sample(first, 12, **kw)
    a.close()
    b_ = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    got, _ = b_.generate_penalized(first, 12, occ, presence=0.0, frequency=0.0, decay=0.996, **kw)
    b_.close()
    assert np.array_equal(got, want)
    w = np.ones(V, np.float32)
    for b in range(B):
        c, f = occ.back(b)
        wc, wf = R.update_all(np.zeros(V, np.float32), np.zeros(V, np.uint32), got[:, b], w, 0.996)
        assert np.array_equal(bits(c), bits(wc)), b
        assert np.array_equal(f, wf), b
    occ.close()


def test_model_level_draws_match_the_restatement(ctx):
    data = model("small")
    V = vocab("small")
    B, k = 3, 10
    T, P, seed = [0.7, 1.0, 1.4], [0.9, 0.6, 1.0], [11, 12, 13]
    ap, af, g = [0.4, 1.5, -0.2], [0.3, 0.0, 0.6], [0.996, 1.0, 0.5]
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    w = np.ones(V, np.float32)
    w[::7] = 0.0
    occ.set_weights(w)
    occ.add(1, [3, 3, 40], 1.0)                       # a counted prompt
    occ.ban(2, [5, 6])
    cur = [7, 100, 900]
    checked = 0
    for step in range(k):       # one-step calls: the draw at t = 0 on the penalised logits of the call
        before = [occ.back(b) for b in range(B)]
        t, _, last = rt.generate_penalized(cur, 1, occ, temperature=T, top_p=P, seed=seed, presence=ap, frequency=af, decay=g,
                                           want_logits=True)
        for b in range(B):
            c, f = before[b]
            x = R.penalize(last[b], c, f, ap[b], af[b]).astype(np.float64)
            args = (x, T[b], P[b], seed[b], 0)
            if not S.ambiguous(*args):
                assert int(t[0, b]) == S.sample(*args), (step, b)
                checked += 1
            wc, wf = R.update(c, f, int(t[0, b]), w, g[b])
            c2, f2 = occ.back(b)
            assert np.array_equal(bits(c2), bits(wc)) and np.array_equal(f2, wf), (step, b)
        assert int(t[0, 2]) not in (5, 6)
        cur = t[0].tolist()
    assert checked >= B * k // 2
    occ.close()
    rt.close()


def repeats_within(toks):
    return len(set(toks)) < len(toks)


def test_greedy_with_a_strong_presence_penalty_never_repeats(ctx):
    data = model("tiny")
    V = vocab("tiny")
    k = 24
    starts = [1, 17, 99, 250, 400]
    rt = fresh(ctx, data, len(starts))
    g, _ = rt.generate_greedy(starts, k)
    rt.close()
    loops = [i for i in range(len(starts)) if repeats_within(g[:, i].tolist())]
    assert loops, "precondition: plain greedy decoding repeats a token within k steps"
    first = starts[loops[0]]
    rt = fresh(ctx, data, 1)
    occ = wrk.Occurrence(ctx, 1, V)
    cur, toks = first, []
    for _ in range(k):
        c, f = occ.back(0)
        t, _, last = rt.generate_penalized([cur], 1, occ, temperature=0.0, presence=1e4, frequency=0.0, want_logits=True)
        assert int(t[0, 0]) == S.greedy(R.penalize(last[0], c, f, 1e4, 0.0))
        cur = int(t[0, 0])
        toks.append(cur)
    assert not repeats_within(toks), toks
    occ.close()
    rt.close()


@pytest.mark.parametrize("v6", [False, True])
def test_the_table_carries_over_between_calls(ctx, v6):
    data = model("tiny", v6)
    V = vocab("tiny", v6)
    B, k = 2, 8
    kw = dict(temperature=0.0, presence=[0.5, 2.0], frequency=[0.3, 0.7], decay=[0.9, 1.0])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    one, _ = rt.generate_penalized([9, 300], 2 * k, occ, **kw)
    rt.close()
    rt = fresh(ctx, data, B)
    occ2 = wrk.Occurrence(ctx, B, V)
    a, _ = rt.generate_penalized([9, 300], k, occ2, **kw)
    b, _ = rt.generate_penalized(a[-1].tolist(), k, occ2, **kw)
    rt.close()
    assert np.array_equal(np.concatenate([a, b]), one)
    for s in range(B):
        c1, f1 = occ.back(s)
        c2, f2 = occ2.back(s)
        assert np.array_equal(bits(c1), bits(c2)) and np.array_equal(f1, f2)
    occ.close()
    occ2.close()


def test_bans(ctx):
    data = model("tiny")
    V = vocab("tiny")
    B = 2
    rt = fresh(ctx, data, B)
    g, _, last = rt.generate_greedy([4, 40], 1, want_logits=True)
    rt.close()
    rng = np.random.default_rng(5)
    banned = [np.unique(np.concatenate([np.argsort(-last[b])[:8], rng.choice(V, 8, replace=False)])) for b in range(B)]
    occ = wrk.Occurrence(ctx, B, V)
    for b in range(B):
        occ.ban(b, banned[b])
        assert np.array_equal(np.flatnonzero(occ.back(b)[1] & R.BANNED), banned[b])
    rt = fresh(ctx, data, B)
    t, _ = rt.generate_penalized([4, 40], 64, occ, temperature=1.0, top_p=1.0)
    rt.close()
    for b in range(B):
        assert not np.isin(t[:, b], banned[b]).any(), b
    # T = 0: the first arg-max of the banned row
    rt = fresh(ctx, data, B)
    cur = [4, 40]
    for _ in range(6):
        before = [occ.back(b) for b in range(B)]
        t, _, last = rt.generate_penalized(cur, 1, occ, temperature=0.0, want_logits=True)
        for b in range(B):
            assert int(t[0, b]) == S.greedy(R.penalize(last[b], *before[b], 0.0, 0.0)), b
        cur = t[0].tolist()
    rt.close()
    # unbanning restores the plain greedy tokens
    for b in range(B):
        occ.ban(b, banned[b], banned=False)
        assert not (occ.back(b)[1] & R.BANNED).any()
    rt = fresh(ctx, data, B)
    t, _ = rt.generate_penalized([4, 40], 8, occ, temperature=0.0)
    rt.close()
    rt = fresh(ctx, data, B)
    want, _ = rt.generate_greedy([4, 40], 8)
    rt.close()
    assert np.array_equal(t, want)
    # a slot must keep at least one allowed token
    with pytest.raises(wrk.WrkError) as e:
        occ.ban(0, np.arange(V))
    assert e.value.code == wrk.E_ARG
    occ.ban(0, np.arange(1, V))
    with pytest.raises(wrk.WrkError) as e:
        occ.ban(0, [0])
    assert e.value.code == wrk.E_ARG
    assert int((occ.back(0)[1] & R.BANNED).sum()) == (V - 1) * R.BANNED
    rt = fresh(ctx, data, B)
    t, _ = rt.generate_penalized([4, 40], 4, occ, temperature=1.0, top_p=1.0)
    rt.close()
    assert (t[:, 0] == 0).all()
    f = np.full(V, R.BANNED, np.uint32)
    with pytest.raises(wrk.WrkError) as e:
        occ.load(1, np.zeros(V, np.float32), f)
    assert e.value.code == wrk.E_ARG
    occ.close()


# ----------------------------------------------------------------------------------------------------------------- captured programs
PEN = dict(temperature=0.8, top_p=0.9, frequency=0.4, decay=0.95)


@pytest.mark.parametrize("B,mode", [(1, 1), (2, 1), (2, 0)])
def test_parameters_and_tables_are_not_baked_into_the_step_program(ctx, B, mode):
    data = model("small")
    V = vocab("small")
    first = [9, 500][:B]
    a = fresh(ctx, data, B)
    greedy_before, _ = a.generate_greedy(first, 8, mode=mode)
    a.close()
    a = fresh(ctx, data, B)
    sample_before, _ = a.generate_sample(first, 8, temperature=1.1, top_p=0.9, mode=mode)
    a.close()

    def zero_state(rt):
        for b in range(B):
            rt.state_load(np.zeros_like(rt.state_back(b)), b)

    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    rt.generate_penalized(first, 8, occ, presence=0.5, mode=mode, **PEN)
    zero_state(rt)
    for b in range(B):
        occ.load(b)
    second, _ = rt.generate_penalized(first, 8, occ, presence=2.0, mode=mode, **PEN)
    second_tab = [occ.back(b) for b in range(B)]
    # the table is data too: destroy it, make a new one, run again
    occ.close()
    zero_state(rt)
    occ_b = wrk.Occurrence(ctx, B, V)
    third, _ = rt.generate_penalized(first, 8, occ_b, presence=2.0, mode=mode, **PEN)
    zero_state(rt)
    greedy_after, _ = rt.generate_greedy(first, 8, mode=mode)
    zero_state(rt)
    sample_after, _ = rt.generate_sample(first, 8, temperature=1.1, top_p=0.9, mode=mode)
    rt.close()
    fr = fresh(ctx, data, B)
    occ_f = wrk.Occurrence(ctx, B, V)
    want, _ = fr.generate_penalized(first, 8, occ_f, presence=2.0, mode=mode, **PEN)
    fr.close()
    assert np.array_equal(second, want)
    assert np.array_equal(third, want)
    for b in range(B):
        cf, ff = occ_f.back(b)
        for c, f in (second_tab[b], occ_b.back(b)):
            assert np.array_equal(bits(c), bits(cf)) and np.array_equal(f, ff)
    assert np.array_equal(greedy_after, greedy_before)
    assert np.array_equal(sample_after, sample_before)
    occ_b.close()
    occ_f.close()


@pytest.mark.parametrize("v6", [False, True])
def test_eager_path_equals_the_replayed_program(ctx, monkeypatch, v6):
    data = model("tiny", v6)
    V = vocab("tiny", v6)
    out = []
    for eager in ("0", "1"):
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
        for mode in (0, 1):
            rt = fresh(ctx, data, 2)
            occ = wrk.Occurrence(ctx, 2, V)
            occ.ban(1, [7, 8, 9])
            out.append(rt.generate_penalized([4, 40], 10, occ, presence=0.3, **PEN, mode=mode)[0])
            out.append(occ.back(0)[0])
            occ.close()
            rt.close()
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], out[4:]))


def test_determinism_and_groups(ctx):
    data = model("small")
    V = vocab("small")
    B = 4
    first = [3, 77, 200, 411]
    kw = dict(temperature=[0.9, 1.1, 1.0, 0.5], top_p=[0.95, 0.8, 1.0, 0.9], presence=[0.2, 0.0, 1.0, 0.5],
              frequency=[0.2, 0.3, 0.0, 0.1], decay=[0.996, 1.0, 0.9, 0.5])
    runs, tabs = [], []
    for _ in range(2):
        rt = fresh(ctx, data, B)
        occ = wrk.Occurrence(ctx, B, V)
        runs.append(rt.generate_penalized(first, 16, occ, **kw)[0])
        tabs.append([occ.back(b) for b in range(B)])
        occ.close()
        rt.close()
    assert np.array_equal(runs[0], runs[1])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    grouped, _ = rt.generate_penalized(first, 16, occ, groups=2, **kw)
    rt.close()
    for b0, b1 in ((0, 2), (2, 4)):
        alone = fresh(ctx, data, b1 - b0)
        occ_a = wrk.Occurrence(ctx, b1 - b0, V)
        t, _ = alone.generate_penalized(first[b0:b1], 16, occ_a, seed=list(range(b0, b1)), **{k: v[b0:b1] for k, v in kw.items()})
        alone.close()
        assert np.array_equal(grouped[:, b0:b1], t)
        assert np.array_equal(runs[0][:, b0:b1], t)
        for b in range(b0, b1):
            c, f = occ.back(b)
            ca, fa = occ_a.back(b - b0)
            assert np.array_equal(bits(c), bits(ca)) and np.array_equal(f, fa)
        occ_a.close()
    occ.close()


# ----------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_the_model_and_table_usable(ctx):
    data = model("tiny")
    V = vocab("tiny")
    rt = fresh(ctx, data, 2)
    occ = wrk.Occurrence(ctx, 2, V)
    occ.add(0, [1, 2, 2], 0.9)
    tab0 = occ.back(0)

    def e_arg(fn, *a, **k):
        with pytest.raises(wrk.WrkError) as e:
            fn(*a, **k)
        assert e.value.code == wrk.E_ARG, e.value

    for bad in (dict(presence=np.nan), dict(presence=np.inf), dict(frequency=-np.inf), dict(frequency=np.nan), dict(decay=np.nan),
                dict(decay=-0.1), dict(decay=1.5), dict(temperature=-1.0)):
        e_arg(rt.generate_penalized, [1, 2], 3, occ, **bad)
    x = np.zeros((2, V), np.float32)
    e_arg(ctx.penalize_logits, x, occ, np.nan, 0.0)
    e_arg(ctx.penalize_logits, x, occ, 0.0, np.inf)
    e_arg(ctx.penalize_logits, x, occ, 0.0, 0.0, first_batch=1)          # slots [1, 3) of 2
    e_arg(ctx.penalize_logits, x[:, :V - 1], occ, 0.0, 0.0)               # another vocabulary
    for w in (np.full(V, -1.0), np.full(V, np.nan), np.full(V, np.inf)):
        e_arg(occ.set_weights, w)
    e_arg(occ.ban, 0, [V])
    e_arg(occ.ban, 2, [1])
    e_arg(occ.add, 0, [1, V], 1.0)
    e_arg(occ.add, 2, [1], 1.0)
    e_arg(occ.add, 0, [1], np.nan)
    e_arg(occ.add, 0, [1], 1.01)
    e_arg(occ.back, 2)
    e_arg(occ.load, 2)
    e_arg(occ.load, 0, np.full(V, np.nan, np.float32), np.zeros(V, np.uint32))
    e_arg(occ.load, 0, np.zeros(V, np.float32), np.full(V, 4, np.uint32))
    e_arg(occ.ban, 0, np.arange(V))
    small = wrk.Occurrence(ctx, 1, V)
    e_arg(rt.generate_penalized, [1, 2], 3, small)                       # fewer slots than sequences
    small.close()
    other_v = wrk.Occurrence(ctx, 2, V + 4)
    e_arg(rt.generate_penalized, [1, 2], 3, other_v)                     # another vocabulary
    other_v.close()
    ctx2 = wrk.Context(0)
    foreign = wrk.Occurrence(ctx2, 2, V)
    e_arg(rt.generate_penalized, [1, 2], 3, foreign)                     # another context
    e_arg(ctx.penalize_logits, x, foreign, 0.0, 0.0)
    assert wrk.hip.wrk_occurrence_ban(ctx.h, foreign.h, 0, wrk._ptr(np.zeros(1, np.uint32), wrk._u32p), 1, 1) == wrk.E_ARG
    foreign.close()
    ctx2.close()
    # NULL arrays and objects through the C ABI
    P_ = wrk._ptr
    ft = np.array([1, 2], np.uint32)
    f = np.ones(2, np.float32)
    z = np.zeros(2, np.float32)
    sd = np.zeros(2, np.uint32)
    out = np.zeros((3, 2), np.uint32)
    fp, up = (lambda a: P_(a, wrk._f32p)), (lambda a: P_(a, wrk._u32p))
    full = [fp(f), fp(f), up(sd), fp(z), fp(z), fp(f), occ.h]
    for i in range(len(full)):
        args = list(full)
        args[i] = None
        rc = wrk.hip.wrk_v7_generate_penalized(ctx.h, rt.model, rt.state, up(ft), 2, 3, *args, up(out), None, None, 1)
        assert rc == wrk.E_ARG, i
    buf = ctx.buffer(x)
    assert wrk.hip.wrk_penalize_logits(ctx.h, buf.h, V, V, 2, occ.h, 0, None, fp(z)) == wrk.E_ARG
    assert wrk.hip.wrk_penalize_logits(ctx.h, buf.h, V, V, 2, None, 0, fp(z), fp(z)) == wrk.E_ARG
    assert wrk.hip.wrk_penalize_logits(ctx.h, buf.h, V, V, 3, occ.h, 0, fp(np.zeros(3, np.float32)), fp(np.zeros(3, np.float32))) == wrk.E_ARG
    assert wrk.hip.wrk_occurrence_ban(ctx.h, occ.h, 0, None, 1, 1) == wrk.E_ARG
    assert wrk.hip.wrk_occurrence_add(ctx.h, occ.h, 0, None, 1, 1.0) == wrk.E_ARG
    assert wrk.hip.wrk_occurrence_back(ctx.h, occ.h, 0, None, up(np.zeros(V, np.uint32))) == wrk.E_ARG
    assert wrk.hip.wrk_occurrence_load(ctx.h, occ.h, 0, fp(np.zeros(V, np.float32)), None) == wrk.E_ARG
    assert wrk.hip.wrk_occurrence_create(ctx.h, 0, V, wrk.C.byref(wrk._P())) == wrk.E_ARG
    # the table is unchanged and the model still runs: greedy equals a fresh runtime's, penalised equals a fresh runtime + table
    c, fl = occ.back(0)
    assert np.array_equal(bits(c), bits(tab0[0])) and np.array_equal(fl, tab0[1])
    assert not occ.back(1)[0].any()
    g, _ = rt.generate_greedy([1, 2], 4)
    fr = fresh(ctx, data, 2)
    assert np.array_equal(g, fr.generate_greedy([1, 2], 4)[0])
    fr.close()
    for b in range(2):
        rt.state_load(np.zeros_like(rt.state_back(b)), b)
        occ.load(b)
    t, _ = rt.generate_penalized([1, 2], 6, occ, presence=0.5, **PEN)
    rt.close()
    fr = fresh(ctx, data, 2)
    occ_f = wrk.Occurrence(ctx, 2, V)
    assert np.array_equal(t, fr.generate_penalized([1, 2], 6, occ_f, presence=0.5, **PEN)[0])
    fr.close()
    occ_f.close()
    occ.close()
