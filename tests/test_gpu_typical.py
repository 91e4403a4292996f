"""Locally typical sampling on the device sampler (web-rwkv-gguf_amd/csrc/wrk_sample.hip `sample_rows_kernel<NPT, SAMPLE_TYP>`)
against the restatement in tests/typical_ref.py: through `Context.sample_logits(typical_p=)`, the decode loops and `generate_queue`.

The kernel test runs the grid of tests/alt_cases.py on four row kinds per vocabulary size (the register variants of one, four and eight
logits per thread, and the L2 path with its odd tail).  A case is excused only where typical_ref says that a prefix mass of the
typical order sits within PREFIX_SLACK of typical_p, that two tokens on opposite sides of gbar are closer in d than f32 can order, or
that u sits on a draw edge."""

import numpy as np
import pytest

import alt_cases as AC
import penalty_ref as R
import typical_ref as TY
import wrk
from oracle.rnn import stack_cursors
from test_gpu_mirostat import FIRST, fresh, model, vocab, zero_states
from test_gpu_queue import MAX_NEW, PROMPT_LENS, Replayer, one, pick, prompts
from test_gpu_sampling import chi2_sf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- 1. the kernel against typical_ref
@pytest.mark.parametrize("V", AC.VOCABS)
def test_kernel_matches_the_restatement(ctx, V):
    clear = total = 0
    for name, l, g, want in AC.typical_expected(V):
        T = np.array([c[0] for c in g], np.float32)
        P = np.array([c[1] for c in g], np.float32)
        seed = np.array([c[2] for c in g], np.uint32)
        buf = ctx.buffer(np.tile(l, (len(g), 1)))
        got = ctx.sample_logits(buf, T, AC.TOP_P, seed, step=AC.STEP, num_vocab=V, typical_p=P)
        assert (got < V).all()
        for i, w in enumerate(want):
            total += 1
            if w is None:
                continue
            clear += 1
            assert int(got[i]) == w, (name, i, g[i], int(got[i]), w)
    assert clear >= 0.95 * total, (clear, total)


# ----------------------------------------------------------------------------- 2. typical_p >= 1 is today's sampler
@pytest.mark.parametrize("V", AC.VOCABS)
def test_typical_p_one_is_the_plain_sampler(ctx, V):
    for name, l, g, _ in AC.typical_expected(V):
        g = g[::3]
        n = len(g)
        T = np.array([c[0] for c in g], np.float32)
        seed = np.array([c[2] for c in g], np.uint32)
        P = np.resize(np.array([0.3, 0.9, 1.0, 0.0], np.float32), n)
        buf = ctx.buffer(np.tile(l, (n, 1)))
        base = ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V)
        assert np.array_equal(ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V, typical_p=1.0), base), name
        ty = np.resize(np.array([1.0, 0.5], np.float32), n)
        mixed = ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V, typical_p=ty)
        assert np.array_equal(mixed[ty >= 1], base[ty >= 1]), name


def test_greedy_branch(ctx):
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (3, 70000)).astype(np.float32)
    x[1, 5] = x[1, 9] = 50.0
    x[2, :] = -np.inf
    assert ctx.sample_logits(x, [0.0, 0.0, 1.0], 0.9, typical_p=0.5).tolist() == [int(x[0].argmax()), 5, 0]


# ----------------------------------------------------------------------------- 3. one candidate
@pytest.mark.parametrize("V", [1, 50, 3000, 6000, 65536])
def test_typical_p_zero_draws_one_token(ctx, V):
    for name, l in AC.rows_for(V)[::3]:
        row = TY.Row(l)
        n = 64
        got = ctx.sample_logits(np.tile(l, (n, 1)), 1.3, 0.0, seed=np.arange(n), step=2, typical_p=0.0)
        assert len(set(got.tolist())) == 1, name
        d = np.sort(row.d)
        if V == 1 or d[1] - d[0] > 2 * TY.gbar_slack(V):        # rank 0 of the typical order is clear of rank 1
            assert int(got[0]) == int(row.torder[0]), name


# ----------------------------------------------------------------------------- 4. distribution
def test_draws_follow_the_candidates_weights(ctx):
    T, P = 0.9, 0.5
    V, n = 1000, 8192
    l = np.random.default_rng(11).normal(0, 1.5, V)
    l = (np.round(l * 4.0) / 4.0).astype(np.float32)       # a flat row, for the distribution only; on a grid so that the set is exact
    row = TY.Row(l)
    toks, c = row.candidates(T, P)
    w = np.diff(np.concatenate([[0.0], c]))
    assert 100 <= len(toks) < V // 2
    got = ctx.sample_logits(np.tile(l, (n, 1)), T, 0.1, seed=np.arange(n, dtype=np.uint32), step=3, typical_p=P)
    assert np.isin(got, toks).all()
    counts = np.bincount(got, minlength=V)[toks]
    expect = w * n
    stat = float(((counts - expect) ** 2 / expect).sum())
    assert chi2_sf(stat, max(len(toks) - 1, 1)) > 1e-6, stat


# ----------------------------------------------------------------------------- 5. the decode loops
TYP = dict(temperature=[0.7, 1.0, 1.4, 0.9], top_p=[0.9, 1.0, 0.0, 0.6], seed=[11, 12, 13, 14], typical_p=[0.9, 0.5, 0.2, 0.95])


def cut(kw, b0, b1):
    return {k: v[b0:b1] for k, v in kw.items()}


def replay(ctx, data, V, B, toks, kw, mode, pen=None, first=None):
    """test_gpu_filter.py's replay with typical_ref.  The replay feeds the device's own tokens and a typical draw carries nothing from
    step to step, so an ambiguous step excuses itself alone: every other step is checked."""
    rt = fresh(ctx, data, B)
    cur = [t % V for t in (first or FIRST[:B])]
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    checked = 0
    for step in range(toks.shape[0]):
        logits = rt.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
        for b in range(B):
            x = logits[b]
            if pen:
                x = R.penalize(x, counts[b], flags[b], pen[0][b], pen[1][b])
                counts[b], flags[b] = R.update(counts[b], flags[b], int(toks[step, b]), ones, pen[2][b])
            row = TY.Row(x)
            args = (kw["temperature"][b], kw["top_p"][b], kw["typical_p"][b], kw["seed"][b], step)
            if row.ambiguous(*args):
                continue
            assert int(toks[step, b]) == row.sample(*args), (step, b)
            checked += 1
        cur = toks[step].tolist()
    rt.close()
    return checked


@pytest.mark.parametrize("cfg,B,mode", [("tiny", 1, 0), ("small", 1, 1), ("small", 4, 1), ("tiny", 4, 0)])
def test_generate_sample_matches_the_replay(ctx, cfg, B, mode):
    data, V = model(cfg), vocab(cfg)
    kw = cut(TYP, 0, B)
    rt = fresh(ctx, data, B)
    toks, _ = rt.generate_sample([t % V for t in FIRST[:B]], 16, mode=mode, **kw)
    rt.close()
    assert replay(ctx, data, V, B, toks, kw, mode) >= 16 * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 0)])
def test_generate_penalized_matches_the_replay(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cut(TYP, 0, B)
    pen = ([0.4, 1.5, -0.2, 0.3][:B], [0.3, 0.0, 0.6, 0.2][:B], [0.996, 1.0, 0.5, 0.9][:B])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    toks, _ = rt.generate_penalized(FIRST[:B], 16, occ, presence=pen[0], frequency=pen[1], decay=pen[2], mode=mode, **kw)
    occ.close()
    rt.close()
    assert replay(ctx, data, V, B, toks, kw, mode, pen) >= 16 * B // 2


def test_v6_generate_sample_matches_the_replay(ctx):
    data, V = model("tiny", True), vocab("tiny", True)
    for mode, kw in ((1, cut(TYP, 0, 2)), (0, cut(TYP, 2, 4))):
        rt = fresh(ctx, data, 2)
        toks, _ = rt.generate_sample([7 % V, 100 % V], 16, mode=mode, **kw)
        rt.close()
        assert replay(ctx, data, V, 2, toks, kw, mode, first=[7, 100]) >= 16


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 0)])
def test_generate_stop_with_typical(ctx, B, mode):
    data = model("small")
    kw = cut(TYP, 0, B)
    rt = fresh(ctx, data, B)
    plain, _ = rt.generate_sample(FIRST[:B], 16, mode=mode, **kw)
    col = plain[:, 0].tolist()
    j = next(j for j in range(3, 16) if col[j] not in col[:j])
    stops = [[col[j]]] + [[] for _ in range(B - 1)]
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 16, stops, mode=mode, poll_steps=4, **kw)
    assert lens.tolist() == [j + 1] + [tok.shape[0]] * (B - 1)
    for b in range(B):
        assert np.array_equal(tok[:lens[b], b], plain[:lens[b], b]), b
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 16, [], mode=mode, **kw)
    assert np.array_equal(tok, plain) and (lens == 16).all() and rt.last_mirostat_mu is None
    rt.close()


# ----------------------------------------------------------------------------- 6. programs
def test_eager_lanes_and_cached_programs(ctx, monkeypatch):
    data = model("small")
    out = []
    for eager in ("0", "1"):
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
        rt = fresh(ctx, data, 2)
        out.append(rt.generate_sample(FIRST[:2], 12, **cut(TYP, 0, 2))[0])
        rt.close()
    assert np.array_equal(out[0], out[1])
    monkeypatch.setenv("WRK_NO_GRAPH", "0")
    monkeypatch.setenv("WRK_ENGINE", "0")
    rt = fresh(ctx, data, 4)
    grouped, _ = rt.generate_sample(FIRST, 12, groups=2, **TYP)
    rt.close()
    for g in range(2):
        rt = fresh(ctx, data, 2)
        alone, _ = rt.generate_sample(FIRST[2 * g:2 * g + 2], 12, **cut(TYP, 2 * g, 2 * g + 2))
        rt.close()
        assert np.array_equal(grouped[:, 2 * g:2 * g + 2], alone), g


@pytest.mark.parametrize("B,mode", [(1, 1), (2, 0)])
def test_parameters_are_data_and_other_programs_are_untouched(ctx, B, mode):
    data = model("small")
    first = FIRST[:B]
    skw = dict(temperature=0.9, top_p=0.9, seed=5)
    rt = fresh(ctx, data, B)

    def four():
        out = []
        for call in (lambda: rt.generate_greedy(first, 8, mode=mode), lambda: rt.generate_sample(first, 8, mode=mode, **skw),
                     lambda: rt.generate_sample(first, 8, mode=mode, top_k=3, min_p=0.1, **skw),
                     lambda: rt.generate_sample(first, 8, mode=mode, mirostat=(1.0, 0.5), **skw),
                     lambda: rt.generate_stop(first, 8, [3], mode=mode, **skw)):
            zero_states(rt, B)
            out.append(call()[0])
        return out
    before = four()
    zero_states(rt, B)
    a, _ = rt.generate_sample(first, 8, mode=mode, typical_p=0.2, **skw)
    zero_states(rt, B)
    b, _ = rt.generate_sample(first, 8, mode=mode, typical_p=0.95, **skw)       # the same step program, other rows
    after = four()
    rt.close()
    other = fresh(ctx, data, B)
    want, _ = other.generate_sample(first, 8, mode=mode, typical_p=0.95, **skw)
    other.close()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.array_equal(b, want) and not np.array_equal(a, b)


# ----------------------------------------------------------------------------- 7. the queue
@pytest.mark.parametrize("kind,B,mode,pool", [("sample", 1, 1, False), ("sample", 2, 1, False), ("pen", 2, 0, False), ("sample", 2, 1, True)])
def test_queue_requests_have_their_own_typical_p(ctx, kind, B, mode, pool):
    data, V = model("small"), vocab("small")
    n = len(PROMPT_LENS)
    reqs = prompts(V)
    kw = pick(kind, n)
    kw["typical_p"] = [[0.9, 0.2, 0.5, 1.0, 0.95, 0.0, 0.7][r] for r in range(n)]
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    if pool:
        pk["pool"] = wrk.StatePool(ctx, rt, 2)
        pk["save_state"] = [0] + [None] * (n - 1)
    res, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **kw, **pk)
    plain, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **{k: v for k, v in kw.items() if k != "typical_p"}, **pk)
    if occ:
        occ.close()
    rt.close()
    rp = Replayer(ctx, data, V, B, kind, mode)
    for r in range(n):
        tokens, reason, slot, _ = res[r]
        assert reason == 2 and len(tokens) == MAX_NEW[r], r
        assert np.array_equal(tokens, rp(slot, reqs[r], [], MAX_NEW[r], one(kw, r))), r
    rp.close()
    assert any(not np.array_equal(res[r][0], plain[r][0]) for r in range(n))
    assert np.array_equal(res[3][0], plain[3][0])          # typical_p == 1: a plain row


# ----------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_leave_the_model_usable(ctx):
    data, V = model("tiny"), vocab("tiny")
    rt = fresh(ctx, data, 2)
    x = np.zeros((2, 16), np.float32)
    for ty in (np.nan, -0.1, 1.5, [0.5, np.inf]):
        for call in (lambda: ctx.sample_logits(x, 1.0, 0.9, typical_p=ty), lambda: rt.generate_sample([1, 2], 3, typical_p=ty),
                     lambda: rt.generate_stop([1, 2], 3, [5], temperature=1.0, typical_p=ty),
                     lambda: rt.generate_queue([[1, 2], [3]], max_new=2, temperature=1.0, typical_p=ty)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG
    for kw in (dict(top_k=3), dict(min_p=0.1)):
        with pytest.raises(wrk.WrkError) as e:
            rt.generate_sample([1, 2], 3, typical_p=0.5, **kw)
        assert e.value.code == wrk.E_ARG
    big = ctx.buffer(np.zeros(2 ** 20 + 1, np.float32))
    with pytest.raises(wrk.WrkError) as e:
        ctx.sample_logits(big, 1.0, 0.9, num_vocab=2 ** 20 + 1, typical_p=0.5)
    assert e.value.code == wrk.E_UNSUPPORTED
    zero_states(rt, 2)
    g, _ = rt.generate_greedy([1, 2], 4)
    other = fresh(ctx, data, 2)
    assert np.array_equal(g, other.generate_greedy([1, 2], 4)[0])
    other.close()
    t, _ = rt.generate_sample([1, 2], 4, temperature=1.0, typical_p=0.5)
    assert t.shape == (4, 2) and (t < V).all()
    rt.close()
