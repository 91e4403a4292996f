"""Mirostat v2 on the device sampler (web-rwkv-gguf_amd/csrc/wrk_sample.hip `sample_rows_kernel<NPT, SAMPLE_MIRO>`) against the
restatement in tests/mirostat_ref.py: through `Context.sample_logits(mirostat=)`, the decode loops (`generate_sample`,
`generate_penalized`, `generate_stop`, RWKV-6) and `generate_queue` with and without a state pool.

The kernel test runs the grid of tests/alt_cases.py on four row kinds per vocabulary size: 1, 50 and 1000 are the one-element register
variant, 3000 and 6000 those of four and eight logits per thread, 16 384 and above re-read the row from L2 (65 529: its odd tail).  A
case is excused only where mirostat_ref says that a surprise sits within the f32 rounding of mu or that u sits on a draw edge; mu is
held to the propagated bound mirostat_ref.mu_tol, summed over the counted draws of a call."""
import ctypes as C
import functools

import numpy as np
import pytest

import alt_cases as AC
import mirostat_ref as M
import penalty_ref as R
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


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- 1. the kernel against mirostat_ref
@pytest.mark.parametrize("V", AC.VOCABS)
def test_kernel_matches_the_restatement(ctx, V):
    clear = total = 0
    for name, l, g, want in AC.mirostat_expected(V):
        T = np.array([c[0] for c in g], np.float32)
        mu = np.array([c[1] for c in g], np.float32)
        seed = np.array([c[2] for c in g], np.uint32)
        buf = ctx.buffer(np.tile(l, (len(g), 1)))
        got, mu2 = ctx.sample_logits(buf, T, AC.TOP_P, seed, step=AC.STEP, num_vocab=V, mirostat=(AC.TAU, AC.ETA, mu))
        assert (got < V).all()
        for i, w in enumerate(want):
            total += 1
            if w is None:
                continue
            clear += 1
            assert int(got[i]) == w[0], (name, i, g[i], int(got[i]), w)
            assert abs(float(mu2[i]) - w[1]) <= w[2], (name, i, g[i], float(mu2[i]), w)
    assert clear >= 0.95 * total, (clear, total)


# ----------------------------------------------------------------------------- 2. tau == 0 is today's sampler
@pytest.mark.parametrize("V", AC.VOCABS)
def test_tau_zero_is_the_plain_sampler(ctx, V):
    for name, l, g, _ in AC.mirostat_expected(V):
        g = g[::3]
        n = len(g)
        T = np.array([c[0] for c in g], np.float32)
        seed = np.array([c[2] for c in g], np.uint32)
        P = np.resize(np.array([0.3, 0.9, 1.0, 0.0], np.float32), n)
        mu = np.resize(np.array([0.5, 7.25, -3.0], np.float32), n)
        buf = ctx.buffer(np.tile(l, (n, 1)))
        base = ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V)
        got, mu2 = ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V, mirostat=(0.0, 0.3, mu))
        assert np.array_equal(got, base), name
        assert np.array_equal(bits(mu2), bits(mu)), name
        # rows of both kinds in one call
        tau = np.resize(np.array([0.0, 5.0], np.float32), n)
        mixed, mu3 = ctx.sample_logits(buf, T, P, seed, step=AC.STEP, num_vocab=V, mirostat=(tau, 0.3, mu))
        assert np.array_equal(mixed[tau == 0], base[tau == 0]) and np.array_equal(bits(mu3[tau == 0]), bits(mu[tau == 0])), name


def test_greedy_branch_leaves_mu_alone(ctx):
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (3, 70000)).astype(np.float32)
    x[1, 5] = x[1, 9] = 50.0
    x[2, :] = -np.inf
    mu = np.array([3.0, 4.0, 5.0], np.float32)
    got, mu2 = ctx.sample_logits(x, [0.0, 0.0, 1.0], 0.9, mirostat=(5.0, 0.1, mu))
    assert got.tolist() == [int(x[0].argmax()), 5, 0] and np.array_equal(bits(mu2), bits(mu))


# ----------------------------------------------------------------------------- 3. one candidate
@pytest.mark.parametrize("V", [1, 50, 3000, 6000, 65536])
def test_mu_below_the_top_surprise_draws_the_argmax(ctx, V):
    l = AC.rows_for(V)[0][1]
    n = 64
    tau, eta, mu = np.float32(5.0), np.float32(0.25), np.float32(-2.0)      # every surprise is >= 0 > mu
    got, mu2 = ctx.sample_logits(np.tile(l, (n, 1)), 1.3, 0.0, seed=np.arange(n), step=2, mirostat=(tau, eta, mu))
    assert (got == int(np.flatnonzero(l == l.max())[0])).all()
    want = np.float32(mu - np.float32(eta * np.float32(np.float32(0.0) - tau)))       # s == 0 exactly: mu moves by -eta (0 - tau)
    assert np.array_equal(bits(mu2), bits(np.full(n, want)))


# ----------------------------------------------------------------------------- 4. distribution
def test_draws_follow_the_candidates_weights(ctx):
    T, mu = 0.9, 8.0
    V, n = 1000, 4096
    l = np.random.default_rng(11).normal(0, 1.5, V).astype(np.float32)      # a flat row: for the distribution only
    got, mu2 = ctx.sample_logits(np.tile(l, (n, 1)), T, 0.1, seed=np.arange(n, dtype=np.uint32), step=3, mirostat=(5.0, 0.1, mu))
    row = M.Row(l, T)
    k = row.count(mu)
    assert not row.count(mu - 1e-3) != row.count(mu + 1e-3) and 2 <= k < V
    toks, w = row.order[:k], row.w[:k] / row.cw[k - 1]
    assert np.isin(got, toks).all()
    counts = np.bincount(got, minlength=V)[toks]
    expect = w * n
    stat = float(((counts - expect) ** 2 / expect).sum())
    assert chi2_sf(stat, max(k - 1, 1)) > 1e-6, stat
    # every row's new mu is the update for the token it drew
    for i in range(0, n, 97):
        r = int(np.flatnonzero(toks == got[i])[0])
        s = np.log2(row.cw[k - 1]) - row.x[r] * M.LOG2E
        assert abs(float(mu2[i]) - (mu - 0.1 * (s - 5.0))) <= M.mu_tol(0.1, 5.0, float(mu2[i]), s, np.log2(row.cw[k - 1]), V)


# ----------------------------------------------------------------------------- 5. the decode loops
MIRO = dict(temperature=[0.7, 1.0, 1.4, 0.9], top_p=[0.9, 1.0, 0.0, 0.6], seed=[11, 12, 13, 14],
            mirostat=([3.0, 5.0, 2.0, 4.0], [0.1, 0.4, 0.2, 1.0]))
FIRST = [7, 100, 900, 411]


def cut(kw, b0, b1):
    return {k: (tuple(x[b0:b1] for x in v) if k == "mirostat" else v[b0:b1]) for k, v in kw.items()}


def replay(ctx, data, V, B, calls, kw, mode, pen=None, first=None):
    """`calls`: [(tokens [k, B], mu after the call [B])] of consecutive Mirostat calls that start from a zero state and a fresh mu, each
    feeding the last tokens and the mu of the one before; step by step through infer's logits and mirostat_ref in f64.  A sequence is
    followed until its first ambiguous step (the threshold slack widened by the bound mu has accumulated).  Checks the tokens of the
    steps followed and, for a sequence followed to the end of a call, its mu inside the accumulated bound.  Returns the draws checked."""
    rt = fresh(ctx, data, B)
    cur = [t % V for t in (first or FIRST[:B])]
    tau, eta = kw["mirostat"]
    mu = [M.start_mu(tau[b]) for b in range(B)]
    tol = [0.0] * B
    live = [True] * B
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    checked = 0
    for toks, mu_dev in calls:
        for step in range(toks.shape[0]):
            logits = rt.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
            for b in range(B):
                x = logits[b]
                if pen:
                    x = R.penalize(x, counts[b], flags[b], pen[0][b], pen[1][b])
                    counts[b], flags[b] = R.update(counts[b], flags[b], int(toks[step, b]), ones, pen[2][b])
                if not live[b]:
                    continue
                row = M.Row(x, kw["temperature"][b])
                if row.ambiguous(mu[b], kw["seed"][b], step, extra=tol[b]):
                    live[b] = False
                    continue
                tok, mu[b], info = row.step(mu[b], tau[b], eta[b], kw["seed"][b], step)
                assert int(toks[step, b]) == tok, (step, b)
                tol[b] += M.mu_tol(eta[b], tau[b], mu[b], info[0], info[1], V)
                checked += 1
            cur = toks[step].tolist()
        for b in range(B):
            if live[b]:
                assert abs(float(mu_dev[b]) - mu[b]) <= tol[b], (b, float(mu_dev[b]), mu[b], tol[b])
    rt.close()
    return checked


@pytest.mark.parametrize("cfg,B,mode", [("tiny", 1, 0), ("small", 1, 1), ("small", 4, 1), ("tiny", 4, 0)])
def test_generate_sample_matches_the_replay(ctx, cfg, B, mode):
    data, V = model(cfg), vocab(cfg)
    kw = cut(MIRO, 0, B)
    first = [t % V for t in FIRST[:B]]
    rt = fresh(ctx, data, B)
    k = 16
    toks, _ = rt.generate_sample(first, k, mode=mode, **kw)
    mu = rt.last_mirostat_mu.copy()
    rt.close()
    assert mu.shape == (B,) and np.isfinite(mu).all()
    assert replay(ctx, data, V, B, [(toks, mu)], kw, mode) >= k * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_generate_penalized_matches_the_replay(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cut(MIRO, 0, B)
    pen = ([0.4, 1.5, -0.2, 0.3][:B], [0.3, 0.0, 0.6, 0.2][:B], [0.996, 1.0, 0.5, 0.9][:B])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    toks, _ = rt.generate_penalized(FIRST[:B], 16, occ, presence=pen[0], frequency=pen[1], decay=pen[2], mode=mode, **kw)
    mu = rt.last_mirostat_mu.copy()
    occ.close()
    rt.close()
    assert replay(ctx, data, V, B, [(toks, mu)], kw, mode, pen) >= 16 * B // 2


def test_v6_generate_sample_matches_the_replay(ctx):
    data, V = model("tiny", True), vocab("tiny", True)
    for mode, kw in ((1, cut(MIRO, 0, 2)), (0, cut(MIRO, 2, 4))):
        rt = fresh(ctx, data, 2)
        toks, _ = rt.generate_sample([7 % V, 100 % V], 16, mode=mode, **kw)
        mu = rt.last_mirostat_mu.copy()
        rt.close()
        assert replay(ctx, data, V, 2, [(toks, mu)], kw, mode, first=[7, 100]) >= 16


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 0)])
def test_mu_is_carried_from_call_to_call(ctx, B, mode):
    """Two calls of 8 steps, the second given the first's last tokens and `last_mirostat_mu`, against one replay that carries mu across
    both (the sampler step restarts at 0 with every call, so the tokens of one 16-step call are other tokens); and the second call
    given no mu starts from 2 tau again."""
    data, V = model("small"), vocab("small")
    kw = cut(MIRO, 0, B)
    rt = fresh(ctx, data, B)
    t1, _ = rt.generate_sample(FIRST[:B], 8, mode=mode, **kw)
    mu1 = rt.last_mirostat_mu.copy()
    state = [rt.state_back(b) for b in range(B)]
    t2, _ = rt.generate_sample(t1[-1], 8, mode=mode, mirostat_mu=mu1, **kw)
    mu2 = rt.last_mirostat_mu.copy()
    for b in range(B):
        rt.state_load(state[b], b)
    t3, _ = rt.generate_sample(t1[-1], 8, mode=mode, **kw)
    mu3 = rt.last_mirostat_mu.copy()
    rt.close()
    assert replay(ctx, data, V, B, [(t1, mu1), (t2, mu2)], kw, mode) >= 8 * B
    assert not np.array_equal(mu1, np.float32(2.0) * np.asarray(kw["mirostat"][0], np.float32))
    assert not np.array_equal(bits(mu2), bits(mu3))


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_generate_stop_counts_the_draws_up_to_the_stop_token(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cut(MIRO, 0, B)
    rt = fresh(ctx, data, B)
    plain, _ = rt.generate_sample(FIRST[:B], 16, mode=mode, **kw)
    mu_plain = rt.last_mirostat_mu.copy()
    col = plain[:, 0].tolist()
    j = next(j for j in range(3, 16) if col[j] not in col[:j])
    stops = [[col[j]]] + [[] for _ in range(B - 1)]
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 16, stops, mode=mode, poll_steps=4, **kw)
    mu_stop = rt.last_mirostat_mu.copy()
    assert lens.tolist() == [j + 1] + [tok.shape[0]] * (B - 1) and tok.shape[0] > j + 1
    for b in range(B):
        assert np.array_equal(tok[:lens[b], b], plain[:lens[b], b]), b
    # mu[0] has seen exactly j + 1 draws: what a call of j + 1 steps leaves; the steps after the stop token left it alone
    zero_states(rt, B)
    rt.generate_sample(FIRST[:B], j + 1, mode=mode, **kw)
    assert bits(rt.last_mirostat_mu)[0] == bits(mu_stop)[0]
    if tok.shape[0] == 16:
        assert np.array_equal(bits(mu_stop[1:]), bits(mu_plain[1:]))
    # without stop ids the options entry point is generate_sample
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 16, [], mode=mode, **kw)
    assert np.array_equal(tok, plain) and (lens == 16).all() and np.array_equal(bits(rt.last_mirostat_mu), bits(mu_plain))
    rt.close()


# ----------------------------------------------------------------------------- 6. programs
def test_eager_path_equals_the_replayed_program(ctx, monkeypatch):
    data = model("tiny")
    out = []
    for eager in ("0", "1"):
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
        rt = fresh(ctx, data, 2)
        toks = rt.generate_sample([4, 40], 16, **cut(MIRO, 0, 2))[0]
        out.append((toks, rt.last_mirostat_mu.copy()))
        tok, lens = rt.generate_stop([4, 40], 16, [int(toks[5, 0])], **cut(MIRO, 0, 2))
        out[-1] += (tok, lens, rt.last_mirostat_mu.copy())
        rt.close()
    for a, b in zip(*out):
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)


def test_tokens_and_mu_do_not_depend_on_the_number_of_lanes(ctx, monkeypatch):
    """The method of test_gpu_filter.py: a lane's block against a call on that block alone."""
    monkeypatch.setenv("WRK_ENGINE", "0")
    data = model("small")
    for groups in (2, 4):
        rt = fresh(ctx, data, 4)
        grouped, _ = rt.generate_sample(FIRST, 12, groups=groups, **MIRO)
        mu = rt.last_mirostat_mu.copy()
        rt.close()
        for g in range(groups):
            b0, b1 = 4 * g // groups, 4 * (g + 1) // groups
            rt = fresh(ctx, data, b1 - b0)
            alone, _ = rt.generate_sample(FIRST[b0:b1], 12, **cut(MIRO, b0, b1))
            assert np.array_equal(grouped[:, b0:b1], alone), (groups, g)
            assert np.array_equal(bits(mu[b0:b1]), bits(rt.last_mirostat_mu)), (groups, g)
            rt.close()


@pytest.mark.parametrize("B,mode", [(1, 1), (2, 0)])
def test_parameters_are_not_baked_into_the_step_program(ctx, B, mode):
    data, V = model("small"), vocab("small")
    first = FIRST[:B]
    a = dict(temperature=1.0, top_p=0.9, seed=3, mirostat=(2.0, 0.5))
    b = dict(temperature=1.0, top_p=0.9, seed=3, mirostat=(6.0, 0.1), mirostat_mu=9.0)
    rt = fresh(ctx, data, B)
    one_, _ = rt.generate_sample(first, 10, mode=mode, **a)
    zero_states(rt, B)
    two, _ = rt.generate_sample(first, 10, mode=mode, **b)             # the same step program, other rows
    mu_two = rt.last_mirostat_mu.copy()
    rt.close()
    other = fresh(ctx, data, B)
    want, _ = other.generate_sample(first, 10, mode=mode, **b)
    assert np.array_equal(two, want) and np.array_equal(bits(mu_two), bits(other.last_mirostat_mu))
    other.close()
    assert not np.array_equal(one_, two)


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 0)])
def test_other_programs_are_untouched_by_a_mirostat_call(ctx, B, mode):
    data = model("small")
    first = FIRST[:B]
    skw = dict(temperature=0.9, top_p=0.9, seed=5)
    rt = fresh(ctx, data, B)

    def four():
        out = []
        zero_states(rt, B)
        out.append(rt.generate_greedy(first, 8, mode=mode)[0])
        zero_states(rt, B)
        out.append(rt.generate_sample(first, 8, mode=mode, **skw)[0])
        zero_states(rt, B)
        out.append(rt.generate_sample(first, 8, mode=mode, top_k=3, min_p=0.1, **skw)[0])
        zero_states(rt, B)
        out.append(rt.generate_stop(first, 8, [3], mode=mode, **skw)[0])
        assert rt.last_mirostat_mu is None
        return out
    before = four()
    zero_states(rt, B)
    miro, _ = rt.generate_sample(first, 8, mode=mode, mirostat=(1.0, 0.5), **skw)
    after = four()
    zero_states(rt, B)
    again, _ = rt.generate_sample(first, 8, mode=mode, mirostat=(1.0, 0.5), **skw)
    rt.close()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert np.array_equal(miro, again)
    assert not np.array_equal(miro, before[1])


# ----------------------------------------------------------------------------- 7. the queue
def queue_kw(kind, n):
    kw = pick(kind, n)
    kw["mirostat"] = [([3.0, 5.0, 2.0, 4.0, 6.0, 1.0, 2.5][r], [0.1, 0.4, 0.2, 1.0, 0.3, 0.5, 0.05][r]) for r in range(n)]
    kw["mirostat_mu"] = [[6.0, 10.0, 1.5, 8.0, 12.0, 2.0, 3.0][r] for r in range(n)]
    return kw


def queue_args(kw):
    q = {k: v for k, v in kw.items() if k not in ("mirostat", "mirostat_mu")}
    q["mirostat"] = ([m[0] for m in kw["mirostat"]], [m[1] for m in kw["mirostat"]])
    q["mirostat_mu"] = kw["mirostat_mu"]
    return q


@pytest.mark.parametrize("kind,B,mode,pool", [("sample", 1, 1, False), ("sample", 2, 1, False), ("pen", 2, 1, False), ("sample", 2, 0, True)])
def test_queue_requests_carry_their_own_mu(ctx, kind, B, mode, pool):
    """Every request against a replay of it alone in its slot: the reply and the final mu do not depend on the slot or the step it was
    scheduled at (B = 1: every request but the first is a refill; B = 2: two slots), and a refilled slot starts from its own request's
    mu, not from its predecessor's."""
    data, V = model("small"), vocab("small")
    n = len(PROMPT_LENS)
    reqs = prompts(V)
    kw = queue_kw(kind, n)
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    if pool:
        pk["pool"] = wrk.StatePool(ctx, rt, 2)
        pk["save_state"] = [0] + [None] * (n - 1)
    res, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **queue_args(kw), **pk)
    mu = rt.last_mirostat_mu.copy()
    if occ:
        occ.close()
    rt.close()
    rp = Replayer(ctx, data, V, B, kind, mode)
    for r in range(n):
        tokens, reason, slot, _ = res[r]
        assert reason == 2 and len(tokens) == MAX_NEW[r], r
        assert np.array_equal(tokens, rp(slot, reqs[r], [], MAX_NEW[r], one(kw, r))), r
        assert bits(rp.rt.last_mirostat_mu)[slot] == bits(mu)[r], r
    rp.close()


def test_queue_mu_of_cut_and_undispatched_requests(ctx):
    data, V = model("small"), vocab("small")
    reqs = prompts(V)[:3]
    kw = queue_kw("sample", 3)
    rt = fresh(ctx, data, 1)
    # one slot, 6 steps: request 0 (prompt 3, 4 new) ends at step 5, request 1 is dispatched by the last step and request 2 never
    res, ran = rt.generate_queue(reqs, max_new=MAX_NEW[:3], max_steps=6, poll_steps=2, **queue_args(kw))
    mu = rt.last_mirostat_mu.copy()
    assert [r[1] for r in res] == [2, 0, 0] and ran == 6
    assert bits(mu)[1] == bits(np.float32(10.0)) and bits(mu)[2] == bits(np.float32(1.5)) and mu[0] != np.float32(6.0)
    # 8 steps: request 1 (prompt 1) has drawn two reply tokens and is cut (reason 3): its mu is that of a 2-token reply
    res, ran = rt.generate_queue(reqs, max_new=MAX_NEW[:3], max_steps=8, poll_steps=2, **queue_args(kw))
    mu = rt.last_mirostat_mu.copy()
    assert [r[1] for r in res] == [2, 3, 0] and len(res[1][0]) == 2
    rt.close()
    rp = Replayer(ctx, data, V, 1, "sample", 1)
    assert np.array_equal(res[1][0], rp(0, reqs[1], [], 2, one(kw, 1)))
    assert bits(rp.rt.last_mirostat_mu)[0] == bits(mu)[1]
    rp.close()


# ----------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_leave_the_model_usable(ctx):
    data, V = model("tiny"), vocab("tiny")
    rt = fresh(ctx, data, 2)
    x = np.zeros((2, 16), np.float32)
    bad = [dict(mirostat=(np.nan, 0.1)), dict(mirostat=(-1.0, 0.1)), dict(mirostat=(np.inf, 0.1)), dict(mirostat=(5.0, np.nan)),
           dict(mirostat=(5.0, -0.1)), dict(mirostat=(5.0, np.inf)), dict(mirostat=(5.0, 0.1), mirostat_mu=np.nan),
           dict(mirostat=(5.0, 0.1), mirostat_mu=[1.0, np.inf]), dict(mirostat=(5.0, 0.1), top_k=3), dict(mirostat=(5.0, 0.1), min_p=0.1),
           dict(mirostat=(5.0, 0.1), typical_p=0.5)]
    for kw in bad:
        calls = [lambda: rt.generate_sample([1, 2], 3, **kw), lambda: rt.generate_stop([1, 2], 3, [5], temperature=1.0, **kw),
                 lambda: rt.generate_queue([[1, 2], [3]], max_new=2, temperature=1.0, **kw)]
        if set(kw) <= {"mirostat", "mirostat_mu"}:
            m = kw["mirostat"] + (kw.get("mirostat_mu"),)
            calls.append(lambda: ctx.sample_logits(x, 1.0, 0.9, mirostat=m))
        for call in calls:
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, kw
    # eta / mu without tau, and a new family without the sampler arrays, through the ABI
    P_ = wrk._ptr
    ft, f2 = np.array([1, 2], np.uint32), np.array([0.5, 0.5], np.float32)
    samp = dict(temperature=P_(f2, wrk._f32p), top_p=P_(f2, wrk._f32p), seed=P_(ft, wrk._u32p))
    out, lens = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32)
    run = C.c_uint32()
    for fields in (dict(samp, mirostat_eta=P_(f2, wrk._f32p)), dict(samp, mirostat_mu=P_(f2, wrk._f32p)), dict(mirostat_tau=P_(f2, wrk._f32p)),
                   dict(typical_p=P_(f2, wrk._f32p)), dict(samp, mirostat_tau=P_(f2, wrk._f32p), typical_p=P_(f2, wrk._f32p))):
        opt = wrk.GenerateOptions()
        for k, v in fields.items():
            setattr(opt, k, v)
        rc = wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p),
                                          P_(lens, wrk._u32p), None, C.byref(run), None, 1)
        assert rc == wrk.E_ARG, list(fields)
        q = wrk.QueueOptions()
        pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
        q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
        for k, v in fields.items():
            setattr(q, k, v)
        arrs = [np.zeros(4, np.uint32) for _ in range(5)]
        res = wrk.QueueResult(*[P_(a, wrk._u32p) for a in arrs], C.pointer(run))
        assert wrk.hip.wrk_v7_generate_queue(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1) == wrk.E_ARG, list(fields)
    big = ctx.buffer(np.zeros(2 ** 20 + 1, np.float32))
    with pytest.raises(wrk.WrkError) as e:
        ctx.sample_logits(big, 1.0, 0.9, num_vocab=2 ** 20 + 1, mirostat=(5.0, 0.1, None))
    assert e.value.code == wrk.E_UNSUPPORTED
    # still usable: the greedy loop from a zero state equals a fresh runtime's, and a Mirostat call runs
    zero_states(rt, 2)
    g, _ = rt.generate_greedy([1, 2], 4)
    other = fresh(ctx, data, 2)
    assert np.array_equal(g, other.generate_greedy([1, 2], 4)[0])
    other.close()
    t, _ = rt.generate_sample([1, 2], 4, temperature=1.0, mirostat=(5.0, 0.1))
    assert t.shape == (4, 2) and (t < V).all() and rt.last_mirostat_mu.shape == (2,)
    rt.close()
