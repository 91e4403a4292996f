"""Log-probs of generated tokens and their top-N alternatives (web-rwkv-gguf_amd/csrc/wrk_logprob.hip) against the f64
restatement in tests/logprob_ref.py: the kernel through `Context.top_logprobs`, then every decode loop through `logprobs=` and
`Runtime.last_logprobs` -- the loop's rows against `last_logits` of shorter calls, lanes, eager steps, scoring, stops, the queue and its
state pool -- and that calls without log-probs are left alone.

Bars.  Kernel log-probs: score_ref.within_bar, the project's bar for this same f32 arithmetic (wrk_score.hip); ids: exact.  Against
`score_sequences`: 2 * LOGIT_TOL of tests/test_gpu_model.py -- the two jobs reach the head through different matmul paths, and a
log-softmax moves by at most twice the largest logit error."""
import ctypes as C
import functools

import numpy as np
import pytest

import logprob_ref as L
import score_ref as R
import test_gpu_queue as TQ
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-2            # tests/test_gpu_model.py's bar on the logits
K = 6                       # steps of the loop tests
NTOP = 5


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=None)
def kernel_case(V, rows):
    """rows, chosen tokens and the restatement with 20 alternatives, computed once per shape (n alternatives are its first n)"""
    x, tok = L.kernel_rows(V, rows, V * 1000 + rows)
    return (x, tok) + L.top_rows(x, tok, L.MAX_TOP)


def check_rows(got, want, n):
    lp, ids, tlp = got
    want_lp, want_ids, want_tlp = want
    assert ids.shape == tlp.shape == (lp.size, n)
    assert (ids.astype(np.int64) == want_ids[:, :n]).all(), np.nonzero((ids != want_ids[:, :n]).any(axis=1))[0][:5]
    ok = R.within_bar(lp, want_lp)
    assert ok.all(), (np.nonzero(~ok)[0][:5], lp[~ok][:5], want_lp[~ok][:5])
    ok = R.within_bar(tlp, want_tlp[:, :n])
    assert ok.all(), (np.argwhere(~ok)[:5], tlp[~ok][:5], want_tlp[:, :n][~ok][:5])


@pytest.mark.parametrize("n", [0, 1, 5, 20])
@pytest.mark.parametrize("rows", [1, 3, 64, 300])
@pytest.mark.parametrize("V", [1, 7, 50, 1000, 65529, 65536])
def test_kernel_matches_the_restatement(ctx, V, rows, n):
    x, tok, *want = kernel_case(V, rows)
    buf = ctx.buffer(x)
    got = ctx.top_logprobs(buf, tok, n, num_vocab=V)
    check_rows(got, want, n)
    lp, ids, tlp = got
    assert same_bits(got, ctx.top_logprobs(buf, tok, n, num_vocab=V))           # fixed reduction order: the same bits on every call
    # the same slicing rule and the same arithmetic as scoring: the same bits
    assert np.array_equal(bits(lp), bits(ctx.score_logits(buf, tok, num_vocab=V)[0]))
    if n:
        greedy = (x.max(axis=1) > -np.inf) & (x.argmax(axis=1) == tok)
        assert greedy.any() or rows < 3
        assert (ids[greedy, 0] == tok[greedy]).all() and np.array_equal(bits(tlp[greedy, 0]), bits(lp[greedy]))
        assert (ids[:, min(V, n):] == L.NO_ID).all() and (tlp[:, min(V, n):] == -np.inf).all()


def test_kernel_strided_rows_and_nan(ctx):
    """Rows of a stride that is not a multiple of 4 (the scalar-load form) with poison in the padding, and a NaN row."""
    V, stride, rows, n = 65529, 65531, 5, 20
    x, tok = L.kernel_rows(V, rows, 5)
    x[3, 17] = np.nan
    buf = np.full((rows, stride), 7.0e3, np.float32)        # padding would dominate every row if it were read
    buf[:, :V] = x
    lp, ids, tlp = ctx.top_logprobs(ctx.buffer(buf), tok, n, num_vocab=V, row_stride=stride)
    assert np.isnan(lp[3]) and np.isnan(tlp[3]).all()
    keep = np.arange(rows) != 3
    want = L.top_rows(x[keep], tok[keep], n)
    check_rows((lp[keep], ids[keep], tlp[keep]), want, n)


def test_kernel_orders_more_than_twenty_equal_maxima_by_index(ctx):
    V, n = 5000, 20
    rng = np.random.default_rng(3)
    x = rng.normal(0.0, 1.0, (2, V)).astype(np.float32)
    at = np.sort(rng.choice(V, 30, replace=False))      # spread over the tile's lanes and waves
    x[:, at] = 9.0
    tok = np.array([at[25], at[0]], np.uint32)          # a maximum outside the alternatives, and the arg-max
    lp, ids, tlp = ctx.top_logprobs(x, tok, n)
    assert (ids == at[:n]).all()
    check_rows((lp, ids, tlp), L.top_rows(x, tok, n), n)
    assert np.array_equal(bits(tlp), np.broadcast_to(bits(lp)[:, None], tlp.shape))


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("V", [5, 1025, 4097])
def test_arg_max_first_alternative_and_rank_zero_are_one_token(ctx, V, pad):
    """The sampler at temperature 0, the first alternative and the scorer's rank 0 name one token, and its log-prob has one bit
    pattern, on rows where a second order or a second expression would show: the maximum 0 held as -0.0 and as +0.0 (in either
    order), next to a NaN and a -inf; stride V + 3 takes the scalar loads."""
    stride, lo, hi = V + pad, V // 2, V - 1
    x = (-np.abs(np.random.default_rng(V).normal(0.0, 2.0, (2, V))) - 0.5).astype(np.float32)
    x[:, 0], x[:, 1] = np.nan, -np.inf
    x[0, lo], x[0, hi] = -0.0, 0.0
    x[1, lo], x[1, hi] = 0.0, -0.0
    for r in x:         # the restatement's order has one answer for these rows
        k = L.keys(r)
        assert np.unique(k).size == V and int(k.argmax()) == lo
        assert np.nonzero(np.nan_to_num(r, nan=-np.inf) == r[lo])[0].tolist() == [lo, hi]
    rows = np.full((2, stride), 7.0e3, np.float32)          # padding would win every row if it were read
    rows[:, :V] = x
    buf = ctx.buffer(rows)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    t, p, seed, tok = np.zeros(2, np.float32), np.full(2, 0.9, np.float32), np.arange(2, dtype=np.uint32), np.full(2, V, np.uint32)
    assert wrk.hip.wrk_sample_logits(ctx.h, buf.h, V, stride, 2, t.ctypes.data_as(f32p), p.ctypes.data_as(f32p), seed.ctypes.data_as(u32p), 0,
                                     tok.ctypes.data_as(u32p)) == 0
    lp, ids, tlp = ctx.top_logprobs(buf, tok, 3, num_vocab=V, row_stride=stride)
    assert tok.tolist() == ids[:, 0].tolist() == [lo] * 2
    score_lp, rank = ctx.score_logits(buf, tok, num_vocab=V, row_stride=stride)
    assert rank.tolist() == [0] * 2
    assert np.array_equal(bits(score_lp), bits(tlp[:, 0])) and np.array_equal(bits(lp), bits(tlp[:, 0]))
    assert np.isnan(score_lp).all()


def test_kernel_rejects_bad_arguments(ctx):
    x = np.zeros((2, 10), np.float32)
    for call in (lambda: ctx.top_logprobs(x, [1, 10], 3), lambda: ctx.top_logprobs(x, [1, 2], wrk.MAX_TOP_LOGPROBS + 1)):
        with pytest.raises(wrk.WrkError) as e:
            call()
        assert e.value.code == wrk.E_ARG
    buf, tok = ctx.buffer(x), np.array([1, 2], np.uint32)
    lp, ids, tlp = np.zeros(2, np.float32), np.zeros(6, np.uint32), np.zeros(6, np.float32)
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def raw(tokens=tok, logprob=lp, top_ids=ids, top_lp=tlp, num_top=3, V=10):
        p = lambda a, ty: None if a is None else a.ctypes.data_as(ty)
        return wrk.hip.wrk_top_logprobs(ctx.h, buf.h, V, V, 2, p(tokens, u32p), num_top, p(logprob, f32p), p(top_ids, u32p), p(top_lp, f32p))
    assert raw() == 0 and raw(top_ids=None, top_lp=None, num_top=0) == 0
    assert [raw(tokens=None), raw(logprob=None), raw(top_ids=None), raw(top_lp=None), raw(V=11)] == [wrk.E_ARG] * 5
    big = ctx.buffer(np.zeros((1, (1 << 20) + 1), np.float32))
    with pytest.raises(wrk.WrkError) as e:
        ctx.top_logprobs(big, [0], 1, num_vocab=(1 << 20) + 1)
    assert e.value.code == wrk.E_UNSUPPORTED


# ------------------------------------------------------------------ 2. the loops see the row last_logits returns
def make_runtime(ctx, version, name, num_batch):
    data = synth.make_v7_gguf(synth.CONFIGS[name], 42) if version == 7 else synth.make_v6_gguf(synth.V6_CONFIGS[name], 42)
    return wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=num_batch)


def reset(rt, occ=None):
    z = np.zeros_like(rt.state_back(0))
    for b in range(rt.num_batch):
        rt.state_load(z, b)
        if occ:
            occ.load(b)


def states(rt):
    return np.stack([rt.state_back(b) for b in range(rt.num_batch)])


def firsts(B, V):
    return [(5 + 61 * b) % V for b in range(B)]


def caller(rt, pick, occ, B):
    """call(steps, **kw) -> the generate_* call of the pick kind on a reset state and table"""
    skw = dict(temperature=[1.0, 0.8, 1.2, 0.9][:B], top_p=[0.9, 1.0, 0.8, 0.95][:B], seed=[11 + b for b in range(B)])
    first = firsts(B, rt.info.num_vocab)

    def call(steps, **kw):
        reset(rt, occ)
        if occ:
            occ.ban(0, [3, 4])          # log-probs are taken before bans: a banned token may be among the alternatives
        if pick == "greedy":
            return rt.generate_greedy(first, steps, **kw)
        if pick == "sample":
            return rt.generate_sample(first, steps, **skw, **kw)
        return rt.generate_penalized(first, steps, occ, presence=0.4, frequency=0.3, decay=0.99, top_k=40, min_p=0.01, **skw, **kw)
    return call


def loop_rows_match_last_logits(ctx, version, name, mode, B, pick):
    rt = make_runtime(ctx, version, name, B)
    V = rt.info.num_vocab
    occ = wrk.Occurrence(ctx, B, V) if pick == "pen" else None
    call = caller(rt, pick, occ, B)
    try:
        tok, _ = call(K, mode=mode, logprobs=NTOP)
        lp, ids, tlp = rt.last_logprobs
        end = states(rt)
        assert lp.shape == (K, B) and ids.shape == tlp.shape == (K, B, NTOP)
        plain, _ = call(K, mode=mode)
        assert rt.last_logprobs is None
        assert np.array_equal(tok, plain) and np.array_equal(bits(end), bits(states(rt)))
        for k in range(1, K + 1):
            t, _, logits = call(k, mode=mode, want_logits=True)
            assert np.array_equal(t, tok[:k])
            check_rows((lp[k - 1], ids[k - 1], tlp[k - 1]), L.top_rows(logits, tok[k - 1], NTOP), NTOP)
        if pick == "greedy":
            assert np.array_equal(ids[..., 0], tok) and np.array_equal(bits(tlp[..., 0]), bits(lp))
    finally:
        if occ:
            occ.close()
        rt.close()


@pytest.mark.parametrize("pick", ["greedy", "sample", "pen"])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("version,name", [(7, "tiny"), (7, "small"), (6, "tiny")])
def test_loop_rows_match_last_logits(ctx, version, name, mode, B, pick):
    loop_rows_match_last_logits(ctx, version, name, mode, B, pick)


@pytest.mark.parametrize("pick", ["greedy", "sample", "pen"])
def test_loop_rows_match_last_logits_engine_off(ctx, monkeypatch, pick):
    monkeypatch.setenv("WRK_ENGINE", "0")
    loop_rows_match_last_logits(ctx, 7, "small", 1, 1, pick)


# ------------------------------------------------------------------ 3. lanes, 4. eager steps
def loop_call(ctx, pick, groups=1, mode=1, B=4, n=NTOP):
    rt = make_runtime(ctx, 7, "small", B)
    try:
        tok, _ = caller(rt, pick, None, B)(K, mode=mode, groups=groups, logprobs=n)
        return (tok,) + rt.last_logprobs
    finally:
        rt.close()


@pytest.mark.parametrize("pick", ["greedy", "sample"])
def test_log_probs_do_not_depend_on_the_number_of_lanes(ctx, pick):
    assert same_bits(loop_call(ctx, pick, groups=1), loop_call(ctx, pick, groups=2))


@pytest.mark.parametrize("pick,B", [("greedy", 1), ("sample", 4)])
def test_eager_steps_give_the_bits_of_replayed_programs(ctx, monkeypatch, pick, B):
    want = loop_call(ctx, pick, B=B)
    monkeypatch.setenv("WRK_NO_GRAPH", "1")
    assert same_bits(want, loop_call(ctx, pick, B=B))


# ------------------------------------------------------------------ 5. agreement with scoring
@pytest.mark.parametrize("version", [7, 6])
def test_log_probs_agree_with_score_sequences(ctx, version):
    B = 2
    rt = make_runtime(ctx, version, "small", B)
    try:
        first = firsts(B, rt.info.num_vocab)
        reset(rt)
        tok, _ = rt.generate_greedy(first, K, logprobs=0)
        lp = rt.last_logprobs[0]
        reset(rt)
        scored = rt.score_sequences([[first[b]] + tok[:, b].tolist() for b in range(B)])
        d = max(np.abs(scored[b][0].astype(np.float64) - lp[:, b]).max() for b in range(B))
        print(f"RWKV-{version}: max |logprob - score_sequences| = {d:.3e} (bar {2 * LOGIT_TOL})")
        assert d <= 2 * LOGIT_TOL
    finally:
        rt.close()


# ------------------------------------------------------------------ 6. stop tokens
@pytest.mark.parametrize("pick", ["greedy", "sample"])
@pytest.mark.parametrize("version", [7, 6])
def test_stop_rows_are_those_of_the_call_without_stops(ctx, version, pick):
    B, steps = 3, 12
    rt = make_runtime(ctx, version, "small", B)
    try:
        V = rt.info.num_vocab
        first = firsts(B, V)
        kw = {} if pick == "greedy" else dict(temperature=[1.0, 0.8, 1.2], top_p=[0.9, 1.0, 0.8], seed=[11, 12, 13])
        reset(rt)
        plain, _ = rt.generate_stop(first, steps, [], logprobs=NTOP, **kw)
        want = rt.last_logprobs
        assert plain.shape[0] == steps
        # sequence 0 ends mid-way on a token that is new there, sequence 1 never, sequence 2 on its first token
        stops = [[TQ.new_at(plain[:, 0], 3)[1]], [], [int(plain[0, 2])]]
        reset(rt)
        tok, lens = rt.generate_stop(first, steps, stops, poll_steps=4, logprobs=NTOP, **kw)
        got, end = rt.last_logprobs, states(rt)
        reset(rt)
        tok0, lens0 = rt.generate_stop(first, steps, stops, poll_steps=4, **kw)
        assert rt.last_logprobs is None
        assert np.array_equal(tok, tok0) and np.array_equal(lens, lens0) and np.array_equal(bits(end), bits(states(rt)))
        assert 3 < lens[0] < steps and lens[1] == tok.shape[0] and lens[2] == 1
        assert got[0].shape == (tok.shape[0], B) and got[1].shape == got[2].shape == (tok.shape[0], B, NTOP)
        for b in range(B):
            n = int(lens[b])
            assert same_bits([g[:n, b] for g in got], [w[:n, b] for w in want]), b      # the stop token's own row included
    finally:
        rt.close()


# ------------------------------------------------------------------ 7. the queue and its state pool
class LogprobReplayer(TQ.Replayer):
    """tests/test_gpu_queue.py's replay of one request alone in its slot, with the log-prob rows of the reply"""

    def __call__(self, slot, prompt, stop, max_new, kw):
        rt, B = self.rt, self.B
        for b in range(B):
            rt.state_load(self.zero, b)
            if self.occ:
                self.reset_row(b)
        first = [(3 + 17 * b) % self.V for b in range(B)]
        for t in prompt[:-1]:
            first[slot] = t
            self.step(first, kw)
        if self.occ:
            self.reset_row(slot)
        first[slot] = prompt[-1]
        stops = [[] for _ in range(B)]
        stops[slot] = list(stop)
        pk = dict(occurrence=self.occ) if self.occ else {}
        tok, lens = rt.generate_stop(first, max_new, stops, mode=self.mode, logprobs=NTOP, **kw, **pk)
        n = int(lens[slot])
        return tok[:n, slot].copy(), [g[:n, slot].copy() for g in rt.last_logprobs]


def plain_results(got):
    return [(t.tolist(), a, b, c) for t, a, b, c in got]


def queue_rows_equal_replays(ctx, kind, B, v6=False, mode=1):
    data, V = TQ.model("small", v6), TQ.vocab("small", v6)
    P, kw = TQ.prompts(V), TQ.pick(kind, TQ.R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    rep = LogprobReplayer(ctx, data, V, B, kind, mode)
    try:
        plain, _ = rt.generate_queue(P, max_new=TQ.MAX_NEW, mode=mode, poll_steps=TQ.POLL, **kw, **pk)
        stops = TQ.forced_stops(plain, V)
        want, want_run = rt.generate_queue(P, stop=stops, max_new=TQ.MAX_NEW, mode=mode, poll_steps=TQ.POLL, **kw, **pk)
        assert rt.last_logprobs is None
        got, run = rt.generate_queue(P, stop=stops, max_new=TQ.MAX_NEW, mode=mode, poll_steps=TQ.POLL, logprobs=NTOP, **kw, **pk)
        rows = rt.last_logprobs
        assert run == want_run and plain_results(got) == plain_results(want)
        assert len(rows) == TQ.R
        for r in range(TQ.R):
            reply, alone = rep(got[r][2], P[r], stops[r], TQ.MAX_NEW[r], TQ.one(kw, r))
            assert reply.tolist() == got[r][0].tolist()
            assert rows[r][0].shape == (len(reply),) and rows[r][1].shape == rows[r][2].shape == (len(reply), NTOP)
            assert same_bits(rows[r], alone), f"request {r}"
    finally:
        rep.close()
        if occ:
            occ.close()
        rt.close()


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("kind", ["greedy", "sample", "pen"])
def test_queue_rows_equal_each_request_alone(ctx, kind, B):
    queue_rows_equal_replays(ctx, kind, B)


def test_queue_rows_equal_each_request_alone_v6(ctx):
    queue_rows_equal_replays(ctx, "sample", 2, v6=True)


def test_queue_stop_ids_outlive_the_log_prob_arrays(ctx):
    """`generate_queue` with stop ids and log-probs together: the stop ids the options point to stay alive next to the log-prob
    arrays, so every request ends where it ends without log-probs (request 0 at its stop token)."""
    rt = make_runtime(ctx, 7, "tiny", 2)
    reqs = [[5, 9], [17], [40, 3, 8], [11]]
    kw = dict(max_new=6, temperature=1.0, top_p=0.9, seed=[1, 2, 3, 4])
    reset(rt)
    free, _ = rt.generate_queue(reqs, **kw)
    stop = int(free[0][0][1])           # the second reply token of request 0
    runs = []
    for lp in (None, 1, wrk.MAX_TOP_LOGPROBS):
        reset(rt)
        res, ran = rt.generate_queue(reqs, stop=[stop], logprobs=lp, **kw)
        runs.append(([t.tolist() for t, *_ in res], [r[1:] for r in res], ran))
    assert runs[0][0][0][-1] == stop and runs[0][1][0][0] == 1 and len(runs[0][0][0]) <= 2
    assert runs[1] == runs[0] and runs[2] == runs[0]
    rt.close()


def test_pool_call_in_place_is_unchanged_and_has_the_rows_of_replays(ctx):
    """Every request starts from and saves to its own entry (start entry == save entry), the entries zero before the call."""
    data, V, B, mode, kind = TQ.model("small"), TQ.vocab("small"), 2, 1, "sample"
    P, kw = TQ.prompts(V), TQ.pick(kind, TQ.R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    rep = LogprobReplayer(ctx, data, V, B, kind, mode)
    own = list(range(TQ.R))
    try:
        out = []
        for logprobs in (None, NTOP):
            pool = wrk.StatePool(ctx, rt, TQ.R)
            got, run = rt.generate_queue(P, max_new=TQ.MAX_NEW, mode=mode, poll_steps=TQ.POLL, pool=pool, start_state=own, save_state=own,
                                         logprobs=logprobs, **kw)
            out.append((plain_results(got), run, rt.last_queue_saved, [bits(pool.back(k)).copy() for k in own], rt.last_logprobs, got))
            pool.close()
        (a, arun, asaved, aentries, arows, _), (b, brun, bsaved, bentries, rows, got) = out
        assert arows is None and a == b and arun == brun and asaved == bsaved == [True] * TQ.R
        assert all(np.array_equal(x, y) for x, y in zip(aentries, bentries))
        for r in range(TQ.R):
            reply, alone = rep(got[r][2], P[r], [], TQ.MAX_NEW[r], TQ.one(kw, r))
            assert reply.tolist() == got[r][0].tolist() and same_bits(rows[r], alone), f"request {r}"
    finally:
        rep.close()
        rt.close()


# ------------------------------------------------------------------ 8. one program serves any n, 9. the other calls are left alone
def test_one_program_serves_any_number_of_alternatives(ctx):
    """n = 0, 3 and 20 on one runtime give what fresh runtimes give, and a call made before them is the same after them (the check of
    tests/test_gpu_queue.py's test_one_program_serves_any_queue); the alternatives of a smaller n are a prefix of a larger n's."""
    B, mode, ns = 2, 1, [0, 3, 20]
    data, V = TQ.model("small"), TQ.vocab("small")
    first = firsts(B, V)
    skw = dict(temperature=[1.0, 0.8], top_p=[0.9, 1.0], seed=[3, 4])

    def run(rt, n):
        reset(rt)
        tok, _ = rt.generate_sample(first, K, mode=mode, logprobs=n, **skw)
        return (tok,) + rt.last_logprobs

    def fresh(n):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        try:
            return run(rt, n)
        finally:
            rt.close()
    want = [fresh(n) for n in ns]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    try:
        reset(rt)
        before, _ = rt.generate_sample(first, K, mode=mode, **skw)
        got = [run(rt, n) for n in ns] + [run(rt, 3)]
        reset(rt)
        after, _ = rt.generate_sample(first, K, mode=mode, **skw)
    finally:
        rt.close()
    assert all(same_bits(g, w) for g, w in zip(got, want + [want[1]]))
    assert np.array_equal(before, after) and np.array_equal(before, got[0][0])
    assert got[1][2].shape == (K, B, 3) and got[2][2].shape == (K, B, 20)
    assert np.array_equal(got[2][2][..., :3], got[1][2]) and np.array_equal(bits(got[2][3][..., :3]), bits(got[1][3]))
    assert np.array_equal(bits(got[0][1]), bits(got[2][1]))


@pytest.mark.parametrize("version", [7, 6])
def test_calls_without_log_probs_are_left_alone(ctx, version):
    B, steps = 3, 8
    rt = make_runtime(ctx, version, "small", B)
    V = rt.info.num_vocab
    occ = wrk.Occurrence(ctx, B, V)
    first = firsts(B, V)
    skw = dict(temperature=[1.0, 0.8, 1.2], top_p=[0.9, 1.0, 0.8], seed=[11, 12, 13])
    pkw = dict(presence=0.3, frequency=0.2, decay=0.996)
    calls = [lambda **kw: rt.generate_greedy(first, steps, want_logits=True, **kw),
             lambda **kw: rt.generate_sample(first, steps, want_logits=True, **skw, **kw),
             lambda **kw: rt.generate_penalized(first, steps, occ, want_logits=True, **skw, **pkw, **kw),
             lambda **kw: rt.generate_stop(first, steps, [[], [9], []], occurrence=occ, want_logits=True, **skw, **pkw, **kw)]

    def loops(**kw):
        out = []
        for call in calls:
            reset(rt, occ)
            res = call(**kw)
            out.append((res[0].copy(), bits(res[-1]).copy(), bits(states(rt)).copy()))
        return out
    try:
        before = loops()
        with_rows = loops(logprobs=2)
        assert rt.last_logprobs is not None
        after = loops()
        assert rt.last_logprobs is None
        for a, b, c in zip(before, with_rows, after):
            assert all(np.array_equal(x, y) for x, y in zip(a, c))
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        occ.close()
        rt.close()


def test_bad_loop_arguments_are_rejected_before_any_launch(ctx):
    B = 2
    rt = make_runtime(ctx, 7, "tiny", B)
    try:
        first = firsts(B, rt.info.num_vocab)
        rt.generate_greedy(first, 3)
        before = states(rt)
        ft = wrk._u32(first)
        out, lens, run = np.zeros((4, B), np.uint32), np.zeros(B, np.uint32), C.c_uint32()
        lp, ids, tlp = np.zeros(4 * B, np.float32), np.zeros(4 * B * 20, np.uint32), np.zeros(4 * B * 20, np.float32)

        def call(num_top, logprob, top_ids, top_lp):
            o = wrk.GenerateOptions()
            o.num_top = num_top
            if logprob is not None:
                o.out_logprob = wrk._ptr(logprob, wrk._f32p)
            if top_ids is not None:
                o.out_top_ids = wrk._ptr(top_ids, wrk._u32p)
            if top_lp is not None:
                o.out_top_logprobs = wrk._ptr(top_lp, wrk._f32p)
            return wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, wrk._ptr(ft, wrk._u32p), B, 4, C.byref(o), wrk._ptr(out, wrk._u32p),
                                                wrk._ptr(lens, wrk._u32p), None, C.byref(run), None, 1)
        bad = [call(21, lp, ids, tlp), call(3, lp, None, tlp), call(3, lp, ids, None), call(0, None, ids, None), call(0, None, None, tlp)]
        assert bad == [wrk.E_ARG] * len(bad), bad
        assert np.array_equal(bits(states(rt)), bits(before))
        assert call(0, lp, None, None) == 0 and call(20, lp, ids, tlp) == 0
        with pytest.raises(ValueError):
            rt.generate_greedy(first, 3, logprobs=21)
        with pytest.raises(ValueError):
            rt.generate_queue([[1, 2]], logprobs=-1)
    finally:
        rt.close()
