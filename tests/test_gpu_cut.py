"""XTC, top-n-sigma and the eta / epsilon cut-offs on the device sampler (web-rwkv-gguf_amd/csrc/wrk_sample.hip
`sample_rows_kernel<NPT, SAMPLE_CUT>`) against the restatement in tests/cut_ref.py: through `Context.sample_logits`, the
decode loops (`generate_sample`, `generate_penalized`, `generate_stop`, `generate_guided`, lanes, the batch-1 engine, eager steps) and
the queues (`generate_queue`, `generate_queue_guided`).

The kernel test runs the whole grid of tests/cut_cases.py on four row kinds per vocabulary size: both sides of every register variant's
limit (1024, 4096 and 8192 tokens) and the L2 path, tight and strided rows.  A case is excused only where cut_ref.ambiguous says a tested
quantity sits within the kernel's derived error bound of its threshold.  The loops are replayed step by step on the host: the row the
pick saw is rebuilt from `infer_raw` (penalised or guided as the call does it) and drawn from by `Context.sample_logits` at the same
step, which must give the loop's token."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cut_cases as CC
import cut_ref as CR
import penalty_ref as R
import wrk
from cut_ref import Cut
from oracle import synth
from oracle.rnn import stack_cursors
from test_gpu_beam import raw_beam
from test_gpu_guided_queue import NEG_LENS, SCALES, negatives
from test_gpu_guided_queue import Replayer as GuidedReplayer
from test_gpu_queue import MAX_NEW, PROMPT_LENS, Replayer, one, pick, prompts
from test_gpu_sampling import chi2_sf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(cfg="tiny", v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS[cfg], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS[cfg], 42)


def vocab(cfg="tiny", v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)[cfg].num_vocab


def fresh(ctx, data, B):
    return wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)


def zero_states(rt, B):
    z = np.zeros_like(rt.state_back(0))
    for b in range(B):
        rt.state_load(z, b)


# ----------------------------------------------------------------------------- 1. the kernel against cut_ref
@pytest.mark.parametrize("layout", ["tight", "strided"])
@pytest.mark.parametrize("V", CC.VOCABS)
def test_kernel_matches_the_restatement(ctx, V, layout):
    clear = total = 0
    every = 1 if layout == "tight" else 3           # the strided rows: every third case, behind a pad that a stray read would pick up
    stride = V if layout == "tight" else V + 3
    for name, l, g, want in CC.expected(V):
        g, want = g[::every], want[::every]
        rows = np.full((len(g), stride), np.inf, np.float32)
        rows[:, :V] = l
        got = ctx.sample_logits(ctx.buffer(rows), step=CC.STEP, num_vocab=V, row_stride=stride, **CC.columns(g))
        assert got.shape == (len(g),) and (got < V).all()
        for i, w in enumerate(want):
            total += 1
            if w is None:
                continue
            clear += 1
            assert int(got[i]) == w, (name, i, g[i], int(got[i]), w)
    assert clear >= 0.95 * total, (clear, total)


# ----------------------------------------------------------------------------- 2. identities
@pytest.mark.parametrize("V", [1, 50, 1025, 4097, 8193, 65536])
def test_cuts_off_is_the_filtered_and_the_plain_kernel(ctx, V):
    for name, l, g, _ in CC.expected(V):
        g = g[::5]
        col = CC.columns(g)
        n = len(g)
        buf = ctx.buffer(np.tile(l, (n, 1)))
        sam = dict(temperature=col["temperature"], top_p=col["top_p"], seed=col["seed"], step=CC.STEP, num_vocab=V)
        filtered = ctx.sample_logits(buf, top_k=col["top_k"], min_p=col["min_p"], **sam)
        plain = ctx.sample_logits(buf, **sam)
        z = np.zeros(n, np.float32)
        offs = [dict(top_n_sigma=z), dict(epsilon_cutoff=z), dict(eta_cutoff=z), dict(xtc=(z, z + 0.1)), dict(xtc=(z + 1.0, z + 0.51)),
                dict(top_n_sigma=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, xtc=(0.0, 0.0))]
        for kw in offs:                             # the cut kernel runs (an array is given) with every cut off
            assert np.array_equal(ctx.sample_logits(buf, top_k=col["top_k"], min_p=col["min_p"], **sam, **kw), filtered), (name, list(kw))
            assert np.array_equal(ctx.sample_logits(buf, **sam, **kw), plain), (name, list(kw))


def test_temperature_zero_and_top_k_one_are_the_argmax(ctx):
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, (7, 70000)).astype(np.float32)
    x[1, 5] = x[1, 9] = 50.0                             # tie: the first index
    x[2, :] = -np.inf                                    # nothing above -3e38: 0
    x[3, :] = -3.2e38
    x[4, 100] = np.inf
    x[5, ::2] = np.nan
    want = ctx.sample_logits(x, 0.0, 0.5).tolist()       # argmax_rows' answer (test_gpu_sampling.py)
    assert want == [int(np.nanargmax(r)) if (np.nan_to_num(r, nan=-np.inf) > -3e38).any() else 0 for r in x]
    cuts = dict(top_n_sigma=1.0, epsilon_cutoff=0.01, eta_cutoff=0.01, xtc=(1.0, 0.0))      # XTC would drop the arg-max if it applied
    assert ctx.sample_logits(x, 0.0, 0.9, seed=np.arange(7), **cuts).tolist() == want
    assert ctx.sample_logits(x, 1.3, 0.0, seed=np.arange(7), **cuts).tolist() == want
    assert ctx.sample_logits(x, 1.3, 0.9, seed=np.arange(7), top_k=1, **cuts).tolist() == want
    small = rng.normal(0, 1, (5, 50)).astype(np.float32)
    assert ctx.sample_logits(small, 0.7, 1.0, top_k=1, **cuts).tolist() == small.argmax(axis=1).tolist()


# ----------------------------------------------------------------------------- 3. XTC's frequency and the draws
def test_xtc_removes_the_top_token_with_its_probability(ctx):
    """p = (.5, .3, .05, ...): with threshold 0.2 two tokens are over it.  At T = 0.02 the draw is the heaviest candidate up to 1e-11:
    token 1 where the coin fell, token 0 where it did not -- the coin of every seed read off the drawn token."""
    V, N, prob, step = 64, 4096, 0.3, 3
    p = np.full(V, 0.15 / (V - 3))
    p[[7, 20, 33]] = 0.5, 0.3, 0.05
    l = np.log(p).astype(np.float32)
    seeds = np.arange(N, dtype=np.uint32) + 1000
    fell = np.array([CR.coin(int(s), step) < float(np.float32(prob)) for s in seeds])
    sd = 5.0 * np.sqrt(N * prob * (1 - prob))
    assert abs(int(fell.sum()) - N * prob) <= sd            # the seeds chosen stay inside, by the reference alone
    got = ctx.sample_logits(np.tile(l, (N, 1)), 0.02, 1.0, seed=seeds, step=step, xtc=(prob, 0.2))
    assert np.isin(got, [7, 20]).all()
    removed = got == 20
    assert abs(int(removed.sum()) - N * prob) <= sd
    assert np.array_equal(removed, fell)                    # the coin is exact: the same rows
    # at T = 0.9 the draws of the rows whose coin fell follow the surviving set's weights, those of the others the whole set's
    cut = Cut(xtc_p=prob, xtc_t=0.2)
    T, K = 0.9, 12
    got = ctx.sample_logits(np.tile(l, (N, 1)), T, 1.0, seed=seeds, step=step, top_k=K, xtc=(prob, 0.2))
    row = CR.Row(l)
    for part, c in ((fell, 0.0), (~fell, 1.0)):
        toks, cum = row.candidates(T, 1.0, K, 0.0, cut, c=c)
        w = np.diff(np.concatenate([[0.0], cum]))
        assert (7 not in toks.tolist()) == (c == 0.0) and np.isin(got[part], toks).all()
        counts = np.bincount(got[part], minlength=V)[toks]
        expect = w * int(part.sum())
        stat = float(((counts - expect) ** 2 / expect).sum())
        assert chi2_sf(stat, max(len(toks) - 1, 1)) > 1e-6, (c, stat)


# ----------------------------------------------------------------------------- 4. the decode loops against a host replay
CUTS = dict(temperature=[0.7, 1.0, 1.4, 0.9], top_p=[0.9, 1.0, 1.0, 0.6], seed=[11, 12, 13, 14], top_k=[40, 0, 0, 30], min_p=[0.02, 0.0, 0.0, 0.0],
            top_n_sigma=[0.0, 1.5, 0.0, 3.0], epsilon_cutoff=[1e-3, 0.0, 0.0, 0.0], eta_cutoff=[0.0, 0.0, 2e-3, 0.0],
            xtc=[(0.5, 0.05), (0.0, 0.1), (1.0, 0.1), (0.6, 0.02)])
FIRST = [7, 100, 900, 411]


def cols(kw, b0, b1):
    """Sequences [b0, b1) of per-sequence keyword arguments, `xtc` as the (probabilities, thresholds) pair the calls take."""
    out = {k: v[b0:b1] for k, v in kw.items() if k != "xtc"}
    if "xtc" in kw:
        out["xtc"] = ([p for p, _ in kw["xtc"][b0:b1]], [t for _, t in kw["xtc"][b0:b1]])
    return out


def cut_of(kw, b):
    return Cut(kw["top_n_sigma"][b], kw["epsilon_cutoff"][b], kw["eta_cutoff"][b], *kw["xtc"][b])


def replay(ctx, data, V, B, toks, kw, mode, pen=None, scale=None, neg_first=None):
    """`toks` [k, B] of a cut call from a zero state, step by step on the host: the row of `infer_raw` -- guided with the partner's row
    (scale), penalised with penalty_ref on counts that start at zero (pen) -- through `Context.sample_logits` at the same step.  A
    sequence is followed until its first ambiguous step, as in test_gpu_filter.py.  Returns the number of draws checked."""
    FB = 2 * B if scale is not None else B
    rt = fresh(ctx, data, FB)
    cur = [t % V for t in FIRST[:B]] + ([t % V for t in neg_first] if scale is not None else [])
    live = [True] * B
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    checked = 0
    for step in range(toks.shape[0]):
        logits = rt.infer_raw(cur, stack_cursors([1] * FB), list(range(FB)), mode=mode)
        if scale is not None:
            logits = ctx.guide_logits(logits, scale)
        for b in range(B):
            x = logits[b]
            if pen:
                x = R.penalize(x, counts[b], flags[b], pen[0][b], pen[1][b])
                counts[b], flags[b] = R.update(counts[b], flags[b], int(toks[step, b]), ones, pen[2][b])
            args = (kw["temperature"][b], kw["top_p"][b], kw["top_k"][b], kw["min_p"][b], cut_of(kw, b), kw["seed"][b], step)
            if live[b] and CR.Row(x).ambiguous(*args):
                live[b] = False
            if live[b]:
                host = ctx.sample_logits(x, step=step, **{k: v[0] if k != "xtc" else (v[0][0], v[1][0]) for k, v in cols(kw, b, b + 1).items()})
                assert int(toks[step, b]) == int(host[0]) == CR.Row(x).sample(*args), (step, b)
                checked += 1
        cur = toks[step].tolist() * (2 if scale is not None else 1)
    rt.close()
    return checked


@pytest.mark.parametrize("cfg,B,mode,v6", [("tiny", 1, 1, False), ("small", 1, 1, False), ("small", 4, 1, False), ("tiny", 4, 0, False),
                                          ("tiny", 2, 1, True), ("tiny", 2, 0, True)])
def test_generate_sample_matches_the_replay(ctx, cfg, B, mode, v6):
    """B = 1, mode 1: the batch-1 engine; mode 0: the op-by-op layer; v6: the other runner through the same driver."""
    data, V = model(cfg, v6), vocab(cfg, v6)
    rt = fresh(ctx, data, B)
    toks, _ = rt.generate_sample([t % V for t in FIRST[:B]], 10, mode=mode, **cols(CUTS, 0, B))
    plain, _ = fresh(ctx, data, B).generate_sample([t % V for t in FIRST[:B]], 10, mode=mode,
                                                   **{k: v for k, v in cols(CUTS, 0, B).items() if k in ("temperature", "top_p", "seed", "top_k", "min_p")})
    rt.close()
    assert replay(ctx, data, V, B, toks, CUTS, mode) >= 10 * B // 2
    assert B < 4 or not np.array_equal(toks, plain)         # the cuts act: the filtered call draws other tokens


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1)])
def test_generate_penalized_matches_the_replay(ctx, B, mode):
    data, V = model("small"), vocab("small")
    pen = ([0.4, 1.5, -0.2, 0.3][:B], [0.3, 0.0, 0.6, 0.2][:B], [0.996, 1.0, 0.5, 0.9][:B])
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V)
    toks, _ = rt.generate_penalized(FIRST[:B], 10, occ, presence=pen[0], frequency=pen[1], decay=pen[2], mode=mode, **cols(CUTS, 0, B))
    occ.close()
    rt.close()
    assert replay(ctx, data, V, B, toks, CUTS, mode, pen) >= 10 * B // 2


@pytest.mark.parametrize("B,mode", [(1, 1), (4, 1), (4, 0)])
def test_generate_stop_with_cuts(ctx, B, mode):
    data, V = model("small"), vocab("small")
    kw = cols(CUTS, 0, B)
    rt = fresh(ctx, data, B)
    plain, _ = rt.generate_sample(FIRST[:B], 12, mode=mode, **kw)
    col = plain[:, 0].tolist()
    j = next(j for j in range(3, 12) if col[j] not in col[:j])
    stops = [[col[j]]] + [[] for _ in range(B - 1)]
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 12, stops, mode=mode, poll_steps=4, **kw)
    assert lens.tolist() == [j + 1] + [tok.shape[0]] * (B - 1)
    for b in range(B):
        assert np.array_equal(tok[:lens[b], b], plain[:lens[b], b]), b
    zero_states(rt, B)
    tok, lens = rt.generate_stop(FIRST[:B], 12, [], mode=mode, **kw)
    assert np.array_equal(tok, plain) and (lens == 12).all()
    rt.close()
    assert replay(ctx, data, V, B, plain, CUTS, mode) >= 12 * B // 2


@pytest.mark.parametrize("v6", [False, True])
def test_generate_guided_matches_the_replay(ctx, v6):
    data, V, B = model("tiny", v6), vocab("tiny", v6), 2
    scale, neg = [1.5, 0.5], [33 % V, 5 % V]
    rt = fresh(ctx, data, 2 * B)
    first = [t % V for t in FIRST[:B]]
    toks, lens = rt.generate_guided(first, 8, scale, negative_first_tokens=neg, mode=1, **cols(CUTS, 0, B))
    rt.close()
    assert (lens == 8).all()
    assert replay(ctx, data, V, B, toks, CUTS, 1, scale=scale, neg_first=neg) >= 8 * B // 2


def test_eager_steps_equal_the_replayed_program(ctx):
    """WRK_NO_GRAPH=1 in a fresh child process: the same tokens from steps that are enqueued one by one."""
    data, V = model("tiny"), vocab("tiny")
    rt = fresh(ctx, data, 2)
    want, _ = rt.generate_sample([4, 40], 10, **cols(CUTS, 0, 2))
    rt.close()
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import numpy as np, wrk, test_gpu_cut as T\n"
            "c = wrk.Context(0); rt = T.fresh(c, T.model('tiny'), 2)\n"
            "print(rt.generate_sample([4, 40], 10, **T.cols(T.CUTS, 0, 2))[0].reshape(-1).tolist())\n"
            "rt.close(); c.close()\n") % (ROOT, os.path.join(ROOT, "web-rwkv-gguf_amd"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, WRK_NO_GRAPH="1"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert eval(out.stdout.strip().splitlines()[-1]) == want.reshape(-1).tolist()


def test_tokens_do_not_depend_on_the_number_of_lanes(ctx, monkeypatch):
    """Each lane's block equals the block run alone (the method of test_gpu_filter.py: lanes keep the five-launch layer)."""
    monkeypatch.setenv("WRK_ENGINE", "0")
    data = model("small")
    for groups in (2, 4):
        rt = fresh(ctx, data, 4)
        grouped, _ = rt.generate_sample(FIRST, 12, groups=groups, **cols(CUTS, 0, 4))
        rt.close()
        for g in range(groups):
            b0, b1 = 4 * g // groups, 4 * (g + 1) // groups
            rt = fresh(ctx, data, b1 - b0)
            alone, _ = rt.generate_sample(FIRST[b0:b1], 12, **cols(CUTS, b0, b1))
            rt.close()
            assert np.array_equal(grouped[:, b0:b1], alone), (groups, g)


def test_cuts_are_not_baked_into_the_step_program(ctx):
    data, V, B = model("small"), vocab("small"), 2
    a = dict(temperature=1.0, top_p=1.0, seed=3, xtc=(1.0, 0.002))      # the synthetic model's rows are flat: p around 1 / V
    b = dict(temperature=1.0, top_p=1.0, seed=3, top_n_sigma=1.0)
    rt = fresh(ctx, data, B)
    one_, _ = rt.generate_sample(FIRST[:B], 10, **a)
    zero_states(rt, B)
    two, _ = rt.generate_sample(FIRST[:B], 10, **b)         # the same step program, other cut rows
    zero_states(rt, B)
    plain, _ = rt.generate_sample(FIRST[:B], 10, temperature=1.0, top_p=1.0, seed=3)
    zero_states(rt, B)
    again, _ = rt.generate_sample(FIRST[:B], 10, **a)
    rt.close()
    other = fresh(ctx, data, B)
    want, _ = other.generate_sample(FIRST[:B], 10, **b)
    other.close()
    assert np.array_equal(two, want) and np.array_equal(one_, again)
    assert not np.array_equal(one_, two) and not np.array_equal(one_, plain)


# ----------------------------------------------------------------------------- 5. the queues
def queue_cuts(n):
    return dict(top_k=[[0, 3, 40, 0, 2, 0, 5][r] for r in range(n)], min_p=[[0.1, 0.0, 0.02, 0.0, 0.0, 0.0, 0.0][r] for r in range(n)],
                top_n_sigma=[[0.0, 2.0, 0.0, 0.0, 1.0, 0.0, 3.0][r] for r in range(n)],
                epsilon_cutoff=[[0.0, 0.0, 1e-3, 0.0, 0.0, 0.02, 0.0][r] for r in range(n)],
                eta_cutoff=[[0.0, 0.0, 0.0, 2e-3, 0.0, 0.0, 0.01][r] for r in range(n)],
                xtc=[[(0.5, 0.05), (0.0, 0.1), (1.0, 0.1), (1.0, 0.02), (0.3, 0.2), (1.0, 0.6), (0.8, 0.01)][r] for r in range(n)])


def as_arrays(kw):
    return {k: v for k, v in kw.items() if k != "xtc"} | dict(xtc=([p for p, _ in kw["xtc"]], [t for _, t in kw["xtc"]]))


@pytest.mark.parametrize("kind,B,mode", [("sample", 2, 1), ("pen", 2, 1), ("sample", 1, 1), ("sample", 4, 0)])
def test_queue_requests_have_their_own_cuts(ctx, kind, B, mode):
    """Each request of `generate_queue` equals the request run alone, bit for bit, with different cut parameters per request."""
    data, V = model("small"), vocab("small")
    n = len(PROMPT_LENS)
    reqs = prompts(V)
    kw = pick(kind, n) | queue_cuts(n)
    rt = fresh(ctx, data, B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    res, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **as_arrays(kw), **pk)
    filt_kw = {k: v for k, v in kw.items() if k not in ("top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc")}
    filt, _ = rt.generate_queue(reqs, max_new=MAX_NEW, mode=mode, poll_steps=4, **filt_kw, **pk)
    if occ:
        occ.close()
    rt.close()
    rp = Replayer(ctx, data, V, B, kind, mode)
    for r in range(n):
        tokens, reason, slot, _ = res[r]
        assert reason == 2 and len(tokens) == MAX_NEW[r], r
        assert np.array_equal(tokens, rp(slot, reqs[r], [], MAX_NEW[r], one(kw, r))), r
    rp.close()
    assert any(not np.array_equal(res[r][0], filt[r][0]) for r in range(n))


def test_guided_queue_requests_have_their_own_cuts(ctx):
    data, V, B = model("small"), vocab("small"), 2
    n = len(PROMPT_LENS)
    P, N = prompts(V), negatives(V)
    kw = pick("sample", n) | queue_cuts(n)
    rt = fresh(ctx, data, 2 * B)
    res, _ = rt.generate_queue_guided(P, N, SCALES, max_new=MAX_NEW, mode=1, poll_steps=4, **as_arrays(kw))
    rt.close()
    rp = GuidedReplayer(ctx, data, V, B, "sample", 1)
    for r in range(n):
        tokens, reason, slot, _ = res[r]
        assert reason == 2 and len(tokens) == MAX_NEW[r], r
        assert np.array_equal(tokens, rp(slot, P[r], N[r], SCALES[r], [], MAX_NEW[r], one(kw, r))), r
    rp.close()


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("v6", [False, True])
def test_host_and_device_dispatch_agree(ctx, v6, guided):
    """The same requests in order and reversed on two slots: the requests the host dispatched at step 0 of one call are dispatched by a
    refill on the device in the other.  A request's reply is equal bit for bit: the dispatch writes its five cut words either way."""
    V, B, n = vocab("small", v6), 2, 5
    lens, max_new = [3, 1, 2, 1, 3], [6, 4, 5, 6, 3]
    P, N = prompts(V, lens), negatives(V, [1, 2, 0, 3, 2])
    S = [1.5, 0.5, 1.0, 2.0, 3.0]
    per = pick("sample", n) | {k: v[:n] for k, v in queue_cuts(7).items()}
    rt = wrk.Runtime(ctx, wrk.GgufReader(model("small", v6)), num_batch=2 * B if guided else B)

    def call(order):
        kw = as_arrays({k: [v[r] for r in order] for k, v in per.items()})
        if guided:
            res, _ = rt.generate_queue_guided([P[r] for r in order], [N[r] for r in order], [S[r] for r in order], max_new=[max_new[r] for r in order],
                                              mode=1, poll_steps=4, **kw)
        else:
            res, _ = rt.generate_queue([P[r] for r in order], max_new=[max_new[r] for r in order], mode=1, poll_steps=4, **kw)
        at = {r: i for i, r in enumerate(order)}
        return [dict(tok=res[at[r]][0].tolist(), reason=res[at[r]][1], start=res[at[r]][3]) for r in range(n)]
    try:
        fwd, rev = call(list(range(n))), call(list(range(n))[::-1])
    finally:
        rt.close()
    assert len({tuple(p["tok"]) for p in fwd}) > 1
    for r in range(n):
        if not guided:      # dispatched by the host at step 0 in order, by the device in reversed order -- or the reverse
            assert (fwd[r]["start"] == 0) == (r < B) and (rev[r]["start"] == 0) == (n - 1 - r < B), (r, fwd[r], rev[r])
        assert fwd[r]["tok"] == rev[r]["tok"] and fwd[r]["reason"] == rev[r]["reason"], (r, fwd[r], rev[r])


# ----------------------------------------------------------------------------- 6. argument errors and refusals
def test_argument_errors_leave_the_model_usable(ctx):
    data, V = model("tiny"), vocab("tiny")
    rt = fresh(ctx, data, 2)
    x = np.zeros((2, 16), np.float32)
    bad = [dict(top_n_sigma=np.nan), dict(top_n_sigma=-1.0), dict(epsilon_cutoff=np.nan), dict(epsilon_cutoff=-0.1), dict(epsilon_cutoff=1.5),
           dict(eta_cutoff=np.nan), dict(eta_cutoff=-0.1), dict(eta_cutoff=1.5), dict(xtc=(np.nan, 0.1)), dict(xtc=(-0.1, 0.1)),
           dict(xtc=(1.5, 0.1)), dict(xtc=(0.5, np.nan)), dict(xtc=(0.5, -0.1)), dict(xtc=(0.5, 1.5)), dict(epsilon_cutoff=[0.1, 2.0])]
    for kw in bad:
        for call in (lambda: ctx.sample_logits(x, 1.0, 0.9, **kw),
                     lambda: rt.generate_sample([1, 2], 3, **kw),
                     lambda: rt.generate_stop([1, 2], 3, [5], temperature=1.0, **kw),
                     lambda: rt.generate_queue([[1, 2], [3]], max_new=2, temperature=1.0, **kw)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, kw
    # one family per call: the cuts with Mirostat or typical are refused by the binding and by the ABI
    for other in (dict(mirostat=(3.0, 0.1, None)), dict(typical_p=0.5)):
        with pytest.raises(ValueError):
            ctx.sample_logits(x, 1.0, 0.9, top_n_sigma=1.0, **other)
    for other in (dict(mirostat=(3.0, 0.1)), dict(typical_p=0.5)):
        for call in (lambda: rt.generate_sample([1, 2], 3, top_n_sigma=1.0, **other),
                     lambda: rt.generate_queue([[1, 2], [3]], max_new=2, temperature=1.0, xtc=(0.5, 0.1), **other)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, other
    # cut arrays without the sampler arrays, one XTC array alone, a NULL cuts
    P_ = wrk._ptr
    ft, ns = np.array([1, 2], np.uint32), np.array([1.0, 1.0], np.float32)
    out, lens = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32)
    run = C.c_uint32()
    for name in ("top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc_probability"):
        opt = wrk.GenerateOptions()
        setattr(opt, name, P_(ns, wrk._f32p))
        rc = wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p),
                                          P_(lens, wrk._u32p), None, C.byref(run), None, 1)
        assert rc == wrk.E_ARG, name
    t = np.ones(2, np.float32)
    opt = wrk.GenerateOptions()
    opt.temperature, opt.top_p, opt.seed, opt.xtc_threshold = P_(t, wrk._f32p), P_(t, wrk._f32p), P_(ft, wrk._u32p), P_(ns, wrk._f32p)
    rc = wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p), P_(lens, wrk._u32p),
                                      None, C.byref(run), None, 1)
    assert rc == wrk.E_ARG
    q = wrk.QueueOptions()
    pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
    q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
    arrs = [np.zeros(4, np.uint32) for _ in range(5)]
    res = wrk.QueueResult(*[P_(a, wrk._u32p) for a in arrs], C.pointer(run))
    assert wrk.hip.wrk_v7_generate_queue_cut(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1, None) == wrk.E_ARG
    qc = wrk.QueueCuts(P_(ns, wrk._f32p), None, None, None, None, None, None)
    assert wrk.hip.wrk_v7_generate_queue_cut(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1, C.byref(qc)) == wrk.E_ARG
    # the vocabulary limit, before any launch: 2^20 + 1 tokens
    with pytest.raises(wrk.WrkError) as e:
        ctx.sample_logits(np.zeros((1, (1 << 20) + 1), np.float32), 1.0, 0.9, top_n_sigma=1.0)
    assert e.value.code == wrk.E_UNSUPPORTED
    assert ctx.sample_logits(np.zeros((1, 1 << 20), np.float32), 1.0, 1.0, top_n_sigma=1.0, xtc=(1.0, 0.0)).tolist() == [(1 << 20) - 1]
    # still usable
    zero_states(rt, 2)
    g, _ = rt.generate_greedy([1, 2], 4)
    other = fresh(ctx, data, 2)
    assert np.array_equal(g, other.generate_greedy([1, 2], 4)[0])
    other.close()
    tk, _ = rt.generate_sample([1, 2], 4, temperature=1.0, top_p=0.9, top_n_sigma=2.0, xtc=(0.5, 0.1))
    assert tk.shape == (4, 2) and (tk < V).all()
    rt.close()


def test_beam_search_refuses_the_cuts(ctx):
    data = model("tiny")
    rt = fresh(ctx, data, 2)
    ns = np.array([1.0], np.float32)
    assert raw_beam(rt, [1], 3, 2, wrk.GenerateOptions()) == wrk.OK
    for name in ("top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc_probability", "xtc_threshold"):
        gen = wrk.GenerateOptions()
        setattr(gen, name, wrk._ptr(ns, wrk._f32p))
        assert raw_beam(rt, [1], 3, 2, gen) == wrk.E_ARG, name
    rt.close()
