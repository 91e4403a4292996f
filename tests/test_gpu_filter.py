"""Top-k and min-p on the device sampler (web-rwkv-gguf_amd/csrc/wrk_sample.hip `sample_rows_kernel<NPT, SAMPLE_FILT>`) against
the restatement in tests/filter_ref.py: through `Context.sample_logits(top_k=, min_p=)`, the decode loops (`generate_sample`,
`generate_penalized`, `generate_stop`) and `generate_queue`.

The kernel test runs the whole grid of tests/filter_cases.py on four row kinds per vocabulary size; V = 3000 and 8000.. are the
register-resident variants of 4 and 8 logits per thread, 16384 and above re-read the row from L2 (65529: its odd tail).  A case is
excused only where filter_ref.ambiguous says the nucleus boundary or the draw sits within sampling_ref's slack; the top-k and the min-p
cut are exact and excuse nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

import filter_cases as FC
import filter_ref as F
import penalty_ref as R
import sampling_ref as S
import wrk
from oracle import synth
from oracle.rnn import stack_cursors
from test_gpu_queue import MAX_NEW, PROMPT_LENS, Replayer, one, pick, prompts
from test_gpu_sampling import chi2_sf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(cfg="small", v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS[cfg], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS[cfg], 42)


def vocab(cfg="small", v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)[cfg].num_vocab


def fresh(ctx, data, B):
    return wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)


def zero_states(rt, B):
    z = np.zeros_like(rt.state_back(0))
    for b in range(B):
        rt.state_load(z, b)


@functools.lru_cache(maxsize=None)
def expected(V):
    return FC.expected(V)


def columns(g):
    T = np.array([c[0] for c in g], np.float32)
    P = np.array([c[1] for c in g], np.float32)
    K = np.array([c[2] for c in g], np.uint32)
    M = np.array([c[3] for c in g], np.float32)
    seed = np.array([c[4] for c in g], np.uint32)
    return T, P, K, M, seed


# ----------------------------------------------------------------------------- 1. the kernel against filter_ref
@pytest.mark.parametrize("V", FC.VOCABS)
def test_kernel_matches_the_restatement(ctx, V):
    clear = total = 0
    for name, l, g, want in expected(V):
        T, P, K, M, seed = columns(g)
        buf = ctx.buffer(np.tile(l, (len(g), 1)))
        got = ctx.sample_logits(buf, T, P, seed, step=FC.STEP, num_vocab=V, top_k=K, min_p=M)
        assert (got < V).all()
        for i, w in enumerate(want):
            total += 1
            if w is None:
                continue
            clear += 1
            assert int(got[i]) == w, (name, i, g[i], int(got[i]), w)
    assert clear >= 0.95 * total, (clear, total)


def test_third_register_variant(ctx):
    """V = 8000: 8 logits per thread (the filtered kernel's third variant; the grid above reaches the other three and the L2 path)."""
    V = 8000
    l = FC.rows_for(V)[1][1]
    row = F.Row(l)
    g = FC.grid(V)[::7]
    T, P, K, M, seed = columns(g)
    got = ctx.sample_logits(np.tile(l, (len(g), 1)), T, P, seed, step=FC.STEP, top_k=K, min_p=M)
    checked = 0
    for i, (t, p, k, m, s) in enumerate(g):
        if not row.ambiguous(t, p, k, m, s, FC.STEP):
            assert int(got[i]) == row.sample(t, p, k, m, s, FC.STEP), (i, g[i])
            checked += 1
    assert checked >= 0.95 * len(g)


# ----------------------------------------------------------------------------- 2. filters off is today's sampler
@pytest.mark.parametrize("V", FC.VOCABS)
def test_filters_off_is_the_plain_sampler(ctx, V):
    P_ = wrk._ptr
    for name, l, g, _ in expected(V):
        g = g[::4]
        T, P, _, _, seed = columns(g)
        n = len(g)
        buf = ctx.buffer(np.tile(l, (n, 1)))
        base = ctx.sample_logits(buf, T, P, seed, step=FC.STEP, num_vocab=V)
        out = np.full(n, 0xffffffff, np.uint32)
        rc = wrk.hip.wrk_sample_logits_filtered(ctx.h, buf.h, V, V, n, P_(T, wrk._f32p), P_(P, wrk._f32p), None, None, P_(seed, wrk._u32p),
                                                FC.STEP, P_(out, wrk._u32p))
        assert rc == wrk.OK and np.array_equal(out, base), name
        off = [dict(top_k=0, min_p=0.0), dict(top_k=0), dict(min_p=0.0), dict(top_k=V), dict(top_k=V + 7, min_p=0.0), dict(top_k=2 ** 32 - 1)]
        for kw in off:
            assert np.array_equal(ctx.sample_logits(buf, T, P, seed, step=FC.STEP, num_vocab=V, **kw), base), (name, kw)


def test_top_k_one_is_the_argmax(ctx):
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (7, 70000)).astype(np.float32)
    x[1, 5] = x[1, 9] = 50.0                             # tie: the first index
    x[2, :] = -np.inf                                    # nothing above -3e38: 0
    x[3, :] = -3.2e38                                    # finite, but nothing above -3e38: 0
    x[4, 100] = np.inf
    x[5, ::2] = np.nan
    want = [int(np.nanargmax(r)) if (np.nan_to_num(r, nan=-np.inf) > -3e38).any() else 0 for r in x]
    assert ctx.sample_logits(x, 0.0, 0.5).tolist() == want                         # argmax_rows' answer (test_gpu_sampling.py)
    for mp in (None, 0.0, 0.3, 1.0):
        assert ctx.sample_logits(x, 1.3, 0.9, seed=np.arange(7), top_k=1, min_p=mp).tolist() == want
    small = rng.normal(0, 1, (5, 50)).astype(np.float32)
    assert ctx.sample_logits(small, 0.7, 1.0, top_k=1).tolist() == small.argmax(axis=1).tolist()


# ----------------------------------------------------------------------------- 3. distribution
def test_draws_follow_the_filtered_candidates(ctx):
    T, P, K, M = 0.9, 0.95, 12, 0.05
    V, n = 1000, 4096
    l = np.random.default_rng(11).normal(0, 1.5, V).astype(np.float32)
    got = ctx.sample_logits(np.tile(l, (n, 1)), T, P, seed=np.arange(n, dtype=np.uint32), step=3, top_k=K, min_p=M)
    toks, w = F.candidates(l, T, P, K, M)
    assert 2 <= len(toks) <= K
    assert np.isin(got, toks).all()
    counts = np.bincount(got, minlength=V)[toks]
    expect = w * n
    stat = float(((counts - expect) ** 2 / expect).sum())
    assert chi2_sf(stat, max(len(toks) - 1, 1)) > 1e-6, stat


# ----------------------------------------------------------------------------- 4. the decode loops
FILT = dict(temperature=[0.7, 1.0, 1.4, 0.9], top_p=[0.9, 1.0, 1.0, 0.6], seed=[11, 12, 13, 14], top_k=[40, 5, 0, 3], min_p=[0.02, 0.0, 0.1, 0.3])
FIRST = [7, 100, 900, 411]


def cut(kw, b0, b1):
    return {k: v[b0:b1] for k, v in kw.items()}


def replay(ctx, data, V, B, toks, kw, mode, pen=None):
    """`toks` [k, B] of a filtered call from a zero state, step by step through infer's logits and filter_ref; pen: (presence, frequency,
    decay) per sequence -- the penalties restated with penalty_ref on counts that start at zero.  A sequence is followed until its
    first ambiguous step, as in test_gpu_sampling.py.  Returns the number of draws checked."""
    rt = fresh(ctx, data, B)
    cur = FIRST[:B]
    cur = [t % V for t in cur]
    live = [True] * B
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
            row = F.Row(x)
            args = (kw["temperature"][b], kw["top_p"][b], kw["top_k"][b], kw["min_p"][b], kw["seed"][b], step)
            if live[b] and row.ambiguous(*args):
                live[b] = False
            if live[b]:
                assert int(toks[step, b]) == row.sample(*args), (step, b)
                checked += 1
        cur = toks[step].tolist()
    rt.close()
    return checked


@pytest.mark.parametrize("cfg,B,mode", [("tiny", 1, 0), ("small", 1, 1), ("small", 4, 1), ("tiny", 4, 0)])
def test_generate_sample_matches_the_replay(ctx, cfg, B, mode):
    data, V = model(cfg), vocab(cfg)
    kw = cut(FILT, 0, B)
    first = [t % V for t in FIRST[:B]]
    rt = fresh(ctx, data, B)
    k = 10
    toks, _ = rt.generate_sample(first, k, mode=mode, **kw)
    # one-step calls: the draw at step 0 on exactly the logits the call returns
    zero_states(rt, B)
    cur, exact = first, 0
    for _ in range(4):
        t, _, last = rt.generate_sample(cur, 1, mode=mode, want_logits=True, **kw)
        for b in range(B):
            row = F.Row(last[b])
            args = (kw["temperature"][b], kw["top_p"][b], kw["top_k"][b], kw["min_p"][b], kw["seed"][b], 0)
            if not row.ambiguous(*args):
                assert int(t[0, b]) == row.sample(*args), b
                exact += 1
        cur = t[0].tolist()
    rt.close()
    assert exact >= 2 * B
    assert replay(ctx, data, V, B, toks, kw, mode) >= k * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_generate_penalized_matches_the_replay(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cut(FILT, 0, B)
    pen = ([0.4, 1.5, -0.2, 0.3][:B], [0.3, 0.0, 0.6, 0.2][:B], [0.996, 1.0, 0.5, 0.9][:B])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    toks, _ = rt.generate_penalized(FIRST[:B], 10, occ, presence=pen[0], frequency=pen[1], decay=pen[2], mode=mode, **kw)
    occ.close()
    rt.close()
    assert replay(ctx, data, V, B, toks, kw, mode, pen) >= 10 * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_generate_stop_with_filters(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cut(FILT, 0, B)
    rt = fresh(ctx, data, B)
    plain, _ = rt.generate_sample(FIRST[:B], 12, mode=mode, **kw)
    # sequence 0 stops at the first token from step 3 on that it has not drawn before; the others never stop
    col = plain[:, 0].tolist()
    j = next(j for j in range(3, 12) if col[j] not in col[:j])
    stops = [[col[j]]] + [[] for _ in range(B - 1)]
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 12, stops, mode=mode, poll_steps=4, **kw)
    assert lens.tolist() == [j + 1] + [tok.shape[0]] * (B - 1)
    for b in range(B):
        assert np.array_equal(tok[:lens[b], b], plain[:lens[b], b]), b
    # without stop ids the options entry point is generate_sample
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 12, [], mode=mode, **kw)
    assert np.array_equal(tok, plain) and (lens == 12).all()
    rt.close()


def test_v6_generate_sample_matches_the_replay(ctx):
    data, V = model("tiny", True), vocab("tiny", True)
    kw = cut(FILT, 0, 2)
    rt = fresh(ctx, data, 2)
    toks, _ = rt.generate_sample([7 % V, 100 % V], 10, mode=1, **kw)
    zero_states(rt, 2)
    again, _ = rt.generate_sample([7 % V, 100 % V], 10, mode=0, **cut(FILT, 2, 4))
    rt.close()
    assert replay(ctx, data, V, 2, toks, kw, 1) >= 10
    kw2 = cut(FILT, 2, 4)
    assert replay(ctx, data, V, 2, again, kw2, 0) >= 10


def test_eager_path_equals_the_replayed_program(ctx, monkeypatch):
    data, V = model("tiny"), vocab("tiny")
    out = []
    for eager in ("0", "1"):
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
        rt = fresh(ctx, data, 2)
        out.append(rt.generate_sample([4, 40], 10, **cut(FILT, 0, 2))[0])
        rt.close()
    assert np.array_equal(out[0], out[1])


def test_tokens_do_not_depend_on_the_number_of_lanes(ctx, monkeypatch):
    """Lane g uploads the filter rows of its own sequences and runs its block as a call on that block alone does (wrk_hip.h: "results
    equal running each block on its own"): the method of test_gpu_sampling.py's test_determinism_and_groups.  Blocks of different
    sizes run different matmul kernels, whose logits need not agree bit for bit, so the runs are compared block by block.  Lanes
    keep the five-launch layer (the persistent engine needs the whole chip), so a one-sequence block is run alone on that layer too."""
    monkeypatch.setenv("WRK_ENGINE", "0")
    data = model("small")
    for groups in (2, 4):
        rt = fresh(ctx, data, 4)
        grouped, _ = rt.generate_sample(FIRST, 12, groups=groups, **FILT)
        rt.close()
        for g in range(groups):
            b0, b1 = 4 * g // groups, 4 * (g + 1) // groups
            rt = fresh(ctx, data, b1 - b0)
            alone, _ = rt.generate_sample(FIRST[b0:b1], 12, **cut(FILT, b0, b1))
            rt.close()
            assert np.array_equal(grouped[:, b0:b1], alone), (groups, g)
    # the filters act in the lanes: the same grouped call without them draws other tokens
    rt = fresh(ctx, data, 4)
    plain, _ = rt.generate_sample(FIRST, 12, groups=2, **{k: v for k, v in FILT.items() if k not in ("top_k", "min_p")})
    rt.close()
    assert not np.array_equal(plain, grouped)


@pytest.mark.parametrize("B,mode", [(1, 1), (2, 1), (2, 0)])
def test_filters_are_not_baked_into_the_step_program(ctx, B, mode):
    data, V = model("small"), vocab("small")
    first = FIRST[:B]
    a = dict(temperature=1.0, top_p=0.95, seed=3, top_k=2, min_p=0.0)
    b = dict(temperature=1.0, top_p=1.0, seed=3, top_k=0, min_p=0.25)      # no nucleus cut: only a draw edge can excuse a step
    rt = fresh(ctx, data, B)
    one_, _ = rt.generate_sample(first, 10, mode=mode, **a)
    zero_states(rt, B)
    two, _ = rt.generate_sample(first, 10, mode=mode, **b)             # the same step program, other filter rows
    rt.close()
    other = fresh(ctx, data, B)
    want, _ = other.generate_sample(first, 10, mode=mode, **b)
    other.close()
    assert np.array_equal(two, want)
    assert not np.array_equal(one_, two)
    for toks, kw in ((one_, a), (two, b)):
        per = {k: [v] * B for k, v in kw.items()}
        assert replay(ctx, data, V, B, toks, per, mode) >= 10 * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_other_programs_are_untouched_by_a_filtered_call(ctx, B, mode):
    data = model("small")
    first = FIRST[:B]
    skw = dict(temperature=0.9, top_p=0.9, seed=5)
    rt = fresh(ctx, data, B)

    def three():
        out = []
        zero_states(rt, B)
        out.append(rt.generate_greedy(first, 8, mode=mode)[0])
        zero_states(rt, B)
        out.append(rt.generate_sample(first, 8, mode=mode, **skw)[0])
        zero_states(rt, B)
        out.append(rt.generate_stop(first, 8, [3], mode=mode, **skw)[0])
        return out
    before = three()
    zero_states(rt, B)
    filtered, _ = rt.generate_sample(first, 8, mode=mode, top_k=3, min_p=0.1, **skw)
    after = three()
    zero_states(rt, B)
    again, _ = rt.generate_sample(first, 8, mode=mode, top_k=3, min_p=0.1, **skw)
    rt.close()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.array_equal(filtered, again)
    assert not np.array_equal(filtered, before[1])


# ----------------------------------------------------------------------------- 5. the queue
@pytest.mark.parametrize("kind,B,mode", [("sample", 2, 1), ("pen", 2, 1), ("sample", 1, 1), ("sample", 4, 0)])
def test_queue_requests_have_their_own_filters(ctx, kind, B, mode):
    data, V = model("small"), vocab("small")
    n = len(PROMPT_LENS)
    reqs = prompts(V)
    kw = pick(kind, n)
    kw |= dict(top_k=[[0, 3, 40, 1, 2, 0, 5][r] for r in range(n)], min_p=[[0.1, 0.0, 0.02, 0.0, 0.3, 0.0, 1.0][r] for r in range(n)])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    res, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **kw, **pk)
    plain_kw = {k: v for k, v in kw.items() if k not in ("top_k", "min_p")}
    plain, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **plain_kw, **pk)
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


# ----------------------------------------------------------------------------- 6. argument errors
def test_argument_errors_leave_the_model_usable(ctx):
    data, V = model("tiny"), vocab("tiny")
    rt = fresh(ctx, data, 2)
    x = np.zeros((2, 16), np.float32)
    for mp in (np.nan, -0.1, 1.5):
        for call in (lambda: ctx.sample_logits(x, 1.0, 0.9, min_p=mp),
                     lambda: ctx.sample_logits(x, 1.0, 0.9, top_k=3, min_p=[0.1, mp]),
                     lambda: rt.generate_sample([1, 2], 3, min_p=mp),
                     lambda: rt.generate_stop([1, 2], 3, [5], temperature=1.0, min_p=mp, top_k=2),
                     lambda: rt.generate_queue([[1, 2], [3]], max_new=2, temperature=1.0, min_p=mp)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG
    # filter arrays without the sampler arrays
    P_ = wrk._ptr
    ft, tk, mp = np.array([1, 2], np.uint32), np.array([3, 3], np.uint32), np.array([0.1, 0.1], np.float32)
    out, lens = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32)
    run = C.c_uint32()
    for fields in (dict(top_k=P_(tk, wrk._u32p)), dict(min_p=P_(mp, wrk._f32p))):
        opt = wrk.GenerateOptions()
        for k, v in fields.items():
            setattr(opt, k, v)
        rc = wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p),
                                          P_(lens, wrk._u32p), None, C.byref(run), None, 1)
        assert rc == wrk.E_ARG
        q = wrk.QueueOptions()
        pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
        q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
        for k, v in fields.items():
            setattr(q, k, v)
        arrs = [np.zeros(4, np.uint32) for _ in range(5)]
        res = wrk.QueueResult(*[P_(a, wrk._u32p) for a in arrs], C.pointer(run))
        rc = wrk.hip.wrk_v7_generate_queue(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1)
        assert rc == wrk.E_ARG
    # any u32 is a valid top_k
    assert ctx.sample_logits(x, 1.0, 0.9, top_k=[2 ** 32 - 1, 2 ** 31]).shape == (2,)
    # still usable: the greedy loop from a zero state equals a fresh runtime's, and a filtered call runs
    zero_states(rt, 2)
    g, _ = rt.generate_greedy([1, 2], 4)
    other = fresh(ctx, data, 2)
    assert np.array_equal(g, other.generate_greedy([1, 2], 4)[0])
    other.close()
    t, _ = rt.generate_sample([1, 2], 4, temperature=1.0, top_p=0.9, top_k=4, min_p=0.05)
    assert t.shape == (4, 2) and (t < V).all()
    rt.close()


# ----------------------------------------------------------------------------- 7. every step kind has a program of its own
KIND_PICKS = ("greedy", "sample", "sample+filter", "pen", "pen+filter")
KIND_TAILS = ("plain", "stop", "queue", "pool")


@pytest.mark.parametrize("v6", [False, True])
def test_every_step_kind_replays_its_own_program(ctx, v6):
    """The key bits of a step program come from one function of its kind (wrk_step_kind::key): one runtime walks all
    {greedy, sampled, sampled + filtered, penalised, penalised + filtered} x {plain, stop, queue, queue + pool} in modes 0 and 1, every
    call from zero state slots and empty occurrence rows, once in order and once in reverse.  A kind that replayed another kind's
    program would draw by another pick or advance by another tail: the second result of every kind must equal its first bit for bit
    (tokens, last logits, lengths, the queue's log).  Across tails: a stop set that never fires draws what the plain call draws, and
    B one-token requests with max_new = steps draw what sequence b of the plain call draws from the same first token -- the identity
    test_gpu_queue.py's replays rest on (slot b, sampler step j for reply token j, state and occurrence row reset at the start).
    Programs stay cached between the passes, so two picks that shared a key would agree with themselves; the parameters separate them.
    The filtered picks run top_k = 1 at temperature 50: their draw is the arg-max whatever the seed (test_top_k_one_is_the_argmax), the
    plain sampler's at that temperature is not.  The penalised picks ban the first token that their unpenalised counterpart draws
    (bans survive the queue's row reset), so a program without the penalise launch draws a banned token.  Hence: sampled + filtered
    equals greedy, which sampled does not; penalised differs from sampled in the first draw; penalised + filtered differs from greedy
    in the first draw and does not change with the seeds."""
    B, steps = 2, 4
    data, V = model("tiny", v6), vocab("tiny", v6)
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    pool = wrk.StatePool(ctx, rt, B)
    first = [7, 100]
    skw = dict(temperature=[0.9, 1.1], top_p=[0.95, 0.9], seed=[21, 22])
    fkw = dict(skw, temperature=50.0, top_p=1.0, top_k=1)
    pkw = dict(presence=0.4, frequency=0.3, decay=0.99)
    picks = {"greedy": {}, "sample": skw, "sample+filter": fkw, "pen": dict(skw, **pkw), "pen+filter": dict(fkw, **pkw)}
    banned_from = {"pen": "sample", "pen+filter": "greedy"}
    unused = {}     # per (mode, pick): an id the plain call does not draw -- a stop set that never fires
    drawn = {}      # per (mode, pick): the first token of every sequence in the plain call

    def run(mode, pick_, tail, seed=None):
        zero_states(rt, B)
        for b in range(B):
            occ.load(b)
            if pick_ in banned_from:
                occ.ban(b, [drawn[mode, banned_from[pick_]][b]])
        kw = dict(picks[pick_], mode=mode)
        if seed is not None:
            kw["seed"] = seed
        if pick_.startswith("pen"):
            kw["occurrence"] = occ
        if tail == "plain":
            fn = rt.generate_greedy if pick_ == "greedy" else rt.generate_penalized if pick_.startswith("pen") else rt.generate_sample
            pen = (kw.pop("occurrence"),) if pick_.startswith("pen") else ()
            tok, _, logits = fn(first, steps, *pen, want_logits=True, **kw)
            unused[mode, pick_] = next(i for i in range(V) if i not in set(tok.reshape(-1).tolist()))
            drawn.setdefault((mode, pick_), tok[0].tolist())
            return tok, logits.view(np.uint32)
        if tail == "stop":
            tok, lens, logits = rt.generate_stop(first, steps, [unused[mode, pick_]], want_logits=True, **kw)
            return tok, lens, logits.view(np.uint32)
        pk = dict(pool=pool, save_state=list(range(B))) if tail == "pool" else {}
        res, ran = rt.generate_queue([[t] for t in first], max_new=steps, **kw, **pk)
        saved = rt.last_queue_saved if tail == "pool" else []
        return np.stack([t for t, *_ in res], axis=1), np.array([r[1:] for r in res]), np.array(saved), ran

    kinds = [(p, t) for p in KIND_PICKS for t in KIND_TAILS]
    try:
        for mode in (0, 1):
            once = {k: run(mode, *k) for k in kinds}
            again = {k: run(mode, *k) for k in reversed(kinds)}
            for k in kinds:
                assert len(once[k]) == len(again[k])
                for x, y in zip(once[k], again[k]):
                    assert np.array_equal(x, y), (mode, k)
            for p in KIND_PICKS:
                plain = once[p, "plain"][0]
                assert plain.shape == (steps, B)
                tok, lens, _ = once[p, "stop"]
                assert np.array_equal(tok, plain) and lens.tolist() == [steps] * B, (mode, p)
                for t in ("queue", "pool"):
                    tok, log, saved, _ = once[p, t]
                    assert np.array_equal(tok, plain), (mode, p, t)
                    assert log.tolist() == [[2, b, 0] for b in range(B)], (mode, p, t)       # ended by max_new, slot b, fed at step 0
                    assert saved.tolist() == [True] * B * (t == "pool"), (mode, p)
            tok = {p: once[p, "plain"][0] for p in KIND_PICKS}
            assert np.array_equal(tok["sample+filter"], tok["greedy"]) and not np.array_equal(tok["sample"], tok["greedy"]), mode
            assert all(tok["pen"][0, b] != tok["sample"][0, b] for b in range(B)), mode
            assert all(tok["pen+filter"][0, b] != tok["greedy"][0, b] for b in range(B)), mode
            assert np.array_equal(run(mode, "pen+filter", "plain", seed=[121, 122])[0], tok["pen+filter"]), mode
    finally:
        pool.close()
        occ.close()
        rt.close()
