"""Guidance in the request queue (web-rwkv-gguf_amd/csrc/wrk_queue.hip advance_queue_guided) through
`Runtime.generate_queue_guided`, against the schedule of tests/guided_queue_ref.py and against a replay of every request on its own
through `Runtime.generate_guided`.  Every comparison is exact: token ids and bit patterns.

The replay of a request runs it alone in the pair the queue gave it (state slots b and B + b of a fresh runtime of 2B slots), with filler
tokens in the other slots.  With n and m the lengths of its prompt and negative prompt and L = max(n, m): L - 1 one-step calls of the
same pick kind on the 2B frame feed the two prompts; in front of the call at t == L - n, respectively t == L - m, the half's slot is
loaded with its start state, so a half that starts late has run on filler until then, as in the queue.  Then `generate_guided` runs from
(p_{n-1}, q_{m-1}) with the request's scale, parameters, stop set and steps = max_new.  A request without a negative prompt leaves its
partner on filler with scale 1.

Shapes: the R = 7 requests of tests/test_gpu_queue.py (prompts of 1 to 5 tokens, its max_new and forced stops) with negative prompts of
NEG_LENS tokens -- m < n, m > n, m == n, m == 0, and s == 1 with a negative prompt -- and SCALES; B in {1, 2, 4} pairs: frames of 2, 4 and
8 sequences, two pairs ending in the same step, idle pairs at the end, a pair serving three and more requests in a row with alternating
late halves.  Every queue call runs after a `generate_greedy` that leaves garbage in all 2B slots: a missed or early reset of a late half
shows in the replies.

Against a vacuous pass: of the five requests with s != 1 (0, 1, 2, 4, 6) at least three must draw another reply than the same request
served with scale 1.  With the prompts and negative prompts below, oracle/rwkv7.py on the CPU (f16 activations, the greedy pick on
guide_ref.mix of the two rows) says all five differ: requests 0, 1, 2, 4 and 6."""
import ctypes as C

import numpy as np
import pytest

import guided_queue_ref as G
import queue_ref as Q
import test_gpu_queue as TQ
import wrk

pytestmark = pytest.mark.gpu

PROMPT_LENS, MAX_NEW, R, POLL = TQ.PROMPT_LENS, TQ.MAX_NEW, TQ.R, TQ.POLL
NEG_LENS = [1, 4, 5, 0, 2, 3, 2]
SCALES = [1.5, 0.5, 2.0, 1.0, 0.0, 1.0, 3.0]
GUIDED = [r for r in range(R) if SCALES[r] != 1.0]
bits, model, vocab, prompts, pick, one, zero_state = TQ.bits, TQ.model, TQ.vocab, TQ.prompts, TQ.pick, TQ.one, TQ.zero_state


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def negatives(V, lens=NEG_LENS, salt=0):
    return [[(101 + salt + 31 * r + 17 * i) % V for i in range(n)] for r, n in enumerate(lens)]


def max_steps_of(P, N, max_new):
    return sum(max(len(p), len(q)) for p, q in zip(P, N)) + sum(max_new)


def plain_rows(res):
    return [(t.tolist(), a, b, c) for t, a, b, c in res]


class Replayer:
    """Replays one request alone in a pair of a runtime of 2B slots whose every slot holds what a fresh runtime holds.  extra(rt, slot, r)
    -> the keyword arguments of `generate_guided` for a feature the case is about, its rows [B] neutral but the pair's; prepare(slot, r)
    sets the slot's rows of the handles the case owns directly in front of `generate_guided`."""

    def __init__(self, ctx, data, V, B, kind, mode, init=None, neg_init=None):
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
        self.occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None             # the pick rows of generate_guided: B wide
        self.feed_occ = wrk.Occurrence(ctx, 2 * B, V) if kind == "pen" else None    # the one-step calls run 2B sequences
        self.V, self.B, self.kind, self.mode, self.init, self.neg_init = V, B, kind, mode, init, neg_init
        self.zero = zero_state(self.rt)
        self.last = None

    def step(self, first, kw):
        if self.kind == "greedy":
            self.rt.generate_greedy(first, 1, mode=self.mode)
        elif self.kind == "sample":
            self.rt.generate_sample(first, 1, mode=self.mode, **kw)
        else:
            self.rt.generate_penalized(first, 1, self.feed_occ, mode=self.mode, **kw)

    def start(self, slot, snapshot):
        if snapshot is None:
            self.rt.state_load(self.zero, slot)
        else:
            self.rt.state_write(snapshot, slot)

    def __call__(self, slot, prompt, neg, scale, stop, max_new, kw, extra=None, prepare=None, r=None):
        rt, B, V = self.rt, self.B, self.V
        for b in range(2 * B):
            rt.state_load(self.zero, b)
        n, m = len(prompt), len(neg)
        L = max(n, m)
        first = [(3 + 17 * b) % V for b in range(2 * B)]
        for t in range(L):                      # step t of the pair's request; the last one is generate_guided's first
            if t == L - n:
                self.start(slot, self.init)
            if m and t == L - m:
                self.start(B + slot, self.neg_init)
            if t >= L - n:
                first[slot] = prompt[t - (L - n)]
            if m and t >= L - m:
                first[B + slot] = neg[t - (L - m)]
            if t < L - 1:
                self.step(first, kw)
        for b in range(B if self.occ else 0):
            self.occ.load(b)
        if prepare:
            prepare(slot, r)
        stops, scales = [[] for _ in range(B)], [1.0] * B
        stops[slot], scales[slot] = list(stop), scale
        pk = dict(occurrence=self.occ) if self.occ else {}
        more = extra(rt, slot, r) if extra else {}
        tok, lens = rt.generate_guided(first[:B], max_new, scales, negative_first_tokens=first[B:], stop=stops, mode=self.mode, **kw, **pk, **more)
        self.last = dict(length=int(lens[slot]), gs=rt.last_grammar_state, lp=rt.last_logprobs, match=rt.last_stop_match, mu=rt.last_mirostat_mu)
        return tok[:lens[slot], slot].copy()

    def close(self):
        for o in (self.occ, self.feed_occ):
            if o:
                o.close()
        self.rt.close()


def check_against_replays(got, steps_run, rep, P, N, S, stops, max_new, kw, B, max_steps, extra=None, prepare=None, each=None):
    replies, ends = [], None
    for r in range(len(P)):
        replies.append(rep(got[r][2], P[r], N[r], S[r], stops[r], max_new[r], one(kw, r), extra, prepare, r))
        if each:
            each(r, got[r][2], rep.last)
        if rep.last["match"] is not None:       # with stop sequences the replay says what ended it: a match (of either kind) or max_new
            ends = (ends or []) + [(len(replies[r]), Q.STOP if int(rep.last["match"][got[r][2]]) != wrk.STOP_MATCH_NONE else Q.MAX_NEW)]
    want, needed = G.run(P, N, replies, stops, max_new, B, ends=ends)
    for r in range(len(P)):
        t, why, slot, start = got[r]
        print(f"request {r}: pair {slot} start {start} reason {why} reply {t.tolist()} replay {replies[r].tolist()}")
        assert t.tolist() == replies[r].tolist(), f"request {r}"
        assert (why, slot, start) == want[r][1:], f"request {r}: {(why, slot, start)} against the schedule {want[r][1:]}"
    print(f"steps_run {steps_run}, needed {needed}, bound {Q.steps_run_bound(needed, POLL, max_steps)}")
    assert steps_run == Q.steps_run(needed, POLL, max_steps)
    assert needed <= steps_run <= Q.steps_run_bound(needed, POLL, max_steps)
    return replies, needed


def replay_identity(ctx, kind, mode, v6, B):
    data, V = model("small", v6), vocab("small", v6)
    P, N, kw = prompts(V), negatives(V), pick(kind, R)
    max_steps = max_steps_of(P, N, MAX_NEW)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        rt.generate_greedy([5] * (2 * B), 3, mode=mode)             # garbage in all 2B slots: the call does not continue from it
        plain, _ = rt.generate_queue_guided(P, N, SCALES, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        assert [len(t) for t, *_ in plain] == MAX_NEW and [why for _, why, *_ in plain] == [Q.MAX_NEW] * R
        stops = TQ.forced_stops(plain, V)
        rt.generate_greedy([9] * (2 * B), 2, mode=mode)
        got, run = rt.generate_queue_guided(P, N, SCALES, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        check_against_replays(got, run, rep, P, N, SCALES, stops, MAX_NEW, kw, B, max_steps)
        # what the shapes are there for
        assert [why for _, why, *_ in got] == [Q.MAX_NEW, Q.MAX_NEW, Q.STOP, Q.MAX_NEW, Q.STOP, Q.MAX_NEW, Q.STOP]
        assert len(got[2][0]) >= 4 and len(got[4][0]) >= 3 and len(got[6][0]) == 1
        rows, _ = G.schedule(PROMPT_LENS, NEG_LENS, [len(t) for t, *_ in got], B)
        late_cond = [r for r in range(R) if rows[r]["start_step"] > rows[r]["dispatch_step"]]
        late_part = [r for r in range(R) if NEG_LENS[r] and rows[r]["neg_start_step"] > rows[r]["dispatch_step"]]
        assert late_cond == [1, 5] and late_part == [0, 4]
        assert any(rows[r]["dispatch_step"] > 0 for r in late_cond) and any(rows[r]["dispatch_step"] > 0 for r in late_part)   # at a refill too
        if B <= 2:
            assert max(sum(1 for g in got if g[2] == b) for b in range(B)) >= 3
        # guidance changed something: against the same requests served with scale 1
        ones, _ = rt.generate_queue_guided(P, N, 1.0, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        changed = [r for r in GUIDED if plain[r][0].tolist() != ones[r][0].tolist()]
        print(f"guidance changed the replies of requests {changed}")
        assert len(changed) >= 3
        for r in set(range(R)) - set(GUIDED):
            assert plain[r][0].tolist() == ones[r][0].tolist(), r
    finally:
        rep.close()
        if occ:
            occ.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 4. replay identity
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("mode,v6", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("kind", ["greedy", "sample", "pen"])
def test_replay_identity(ctx, kind, mode, v6, B):
    replay_identity(ctx, kind, mode, v6, B)


def test_replay_identity_eager(ctx, monkeypatch):
    monkeypatch.setenv("WRK_NO_GRAPH", "1")
    replay_identity(ctx, "pen", 1, False, 2)


# ----------------------------------------------------------------------------------------------------------------- 5. one dispatch rule
@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("family", ["mirostat", "filtered"])
def test_host_and_device_dispatch_agree(ctx, v6, family):
    """The same five requests in order and in reversed order on two pairs: the requests that the host dispatched at step 0 of one call
    are dispatched by a refill on the device in the other, and the other way round.  With penalties, prompt intake, stop ids and stop
    sequences on, a request's reply, reason, final mu and match word are equal bit for bit."""
    V, B, n = vocab("small", v6), 2, 5
    lens, neg_lens, scales, max_new = [3, 1, 2, 1, 3], [1, 3, 0, 2, 4], [1.5, 0.5, 1.0, 2.0, 0.0], [6, 4, 5, 6, 3]
    P, N = prompts(V, lens), negatives(V, neg_lens)
    per = pick("pen", n) | dict(count_prompt=[0, 1, 0, 0, 2])
    if family == "mirostat":
        tau = [3.0, 2.5, 4.0, 3.5, 2.0]
        per |= dict(mirostat_mu=[2 * t + 0.25 * r for r, t in enumerate(tau)])
        family_kw = lambda order: dict(mirostat=([tau[r] for r in order], [0.1 + 0.05 * r for r in order]))
    else:
        per |= dict(top_k=[40, 5, 200, 17, 3], min_p=[0.0, 0.02, 0.0, 0.01, 0.05])
        family_kw = lambda order: {}
    rt = wrk.Runtime(ctx, wrk.GgufReader(model("small", v6)), num_batch=2 * B)
    occ = wrk.Occurrence(ctx, B, V)

    def call(order, stop, seqs):
        for b in range(B):
            occ.load(b)
        kw = {k: [v[r] for r in order] for k, v in per.items()} | family_kw(order)
        rt.generate_greedy([5] * (2 * B), 2)
        res, _ = rt.generate_queue_guided([P[r] for r in order], [N[r] for r in order], [scales[r] for r in order], stop=[stop[r] for r in order],
                                          max_new=[max_new[r] for r in order], mode=1, poll_steps=POLL, occurrence=occ,
                                          stop_sequences=None if seqs is None else [seqs[r] for r in order], **kw)
        mu, match = rt.last_mirostat_mu, rt.last_stop_match
        at = {r: i for i, r in enumerate(order)}
        return [dict(tok=res[at[r]][0].tolist(), reason=res[at[r]][1], start=res[at[r]][3], mu=None if mu is None else int(bits(mu[at[r]])),
                     match=None if match is None else int(match[at[r]])) for r in range(n)]
    try:
        plain = call(list(range(n)), [[]] * n, None)
        assert all(len(p["tok"]) == m for p, m in zip(plain, max_new))
        stop, seqs = [[] for _ in range(n)], [[] for _ in range(n)]
        stop[0], seqs[4] = [plain[0]["tok"][2]], [plain[4]["tok"][:2]]
        fwd, rev = call(list(range(n)), stop, seqs), call(list(range(n))[::-1], stop, seqs)
    finally:
        occ.close()
        rt.close()
    assert fwd[0]["reason"] == Q.STOP and fwd[4]["reason"] == Q.STOP and fwd[4]["match"] == 0 and len(fwd[4]["tok"]) == 2
    assert len({tuple(p["tok"]) for p in fwd}) > 1
    for r in range(n):
        # dispatched by the host (f = 0: the half that is on time starts at step 0) in one order, by the device in the other
        f_fwd, f_rev = (fwd[r]["start"] - max(0, neg_lens[r] - lens[r]) == 0), (rev[r]["start"] - max(0, neg_lens[r] - lens[r]) == 0)
        assert f_fwd == (r < B) and f_rev == (n - 1 - r < B), (r, fwd[r], rev[r])
        assert {k: v for k, v in fwd[r].items() if k != "start"} == {k: v for k, v in rev[r].items() if k != "start"}, (r, fwd[r], rev[r])


# ----------------------------------------------------------------------------------------------------------------- 6. composition
def composed(ctx, kind, queue_kw, extra, prepare=None, each=None, init=None, neg_init=None, replay=True):
    """The seven requests on B = 2 pairs with one more feature: the queue's replies against their replays through generate_guided
    (replay=False: the queue call alone, for a comparison between two of them)."""
    data, V, B, mode = model("small"), vocab("small"), 2, 1
    P, N, kw = prompts(V), negatives(V), pick(kind, R)
    stops = [[] for _ in range(R)]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
    rep = Replayer(ctx, data, V, B, kind, mode, init=init, neg_init=neg_init) if replay else None
    try:
        rt.generate_greedy([5] * (2 * B), 3, mode=mode)
        got, run = rt.generate_queue_guided(P, N, SCALES, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **queue_kw(rt))
        if replay:
            check_against_replays(got, run, rep, P, N, SCALES, stops, MAX_NEW, kw, B, max_steps_of(P, N, MAX_NEW), extra, prepare,
                                  (lambda r, slot, last: each(rt, r, slot, last)) if each else None)
        return got, rt.last_logprobs
    finally:
        if rep:
            rep.close()
        rt.close()


def rows_of(B, slot, value, neutral):
    out = [neutral] * B
    out[slot] = value
    return out


def test_composes_with_a_grammar(ctx):
    V = vocab("small")
    # two states, every token allowed: an odd token id toggles the state, so the final state depends on the whole reply; state 1 of the
    # second table bans the even ids, so the mask changes replies
    gram = wrk.Grammar(ctx, V, np.arange(V) % 2, [[0, 1], [wrk.GRAMMAR_REJECT, 0]])
    start = [r % 2 for r in range(R)]
    final = {}
    try:
        def each(rt, r, slot, last):
            final[r] = int(last["gs"][slot])
        got, _ = composed(ctx, "sample", lambda rt: dict(grammar=gram, grammar_state=start),
                          lambda rt, slot, r: dict(grammar=gram, grammar_state=rows_of(2, slot, start[r], 0)), each=each)
    finally:
        gram.close()
    assert len(final) == R


def test_composes_with_a_window_and_prompt_intake(ctx):
    V, B = vocab("small"), 2
    win, rwin = wrk.TokenWindow(ctx, B, V, 8), wrk.TokenWindow(ctx, B, V, 8)
    P = prompts(V)
    frm = [0, 1, 2, 0, 1, 0, 5]
    dry = ([3.0, 0.0, 25.0, 40.0, 3.0, 2.0, 0.0], [1.75, 1.75, 2.0, 1.75, 1e30, 1.5, 1.0], [1, 2, 1, 1, 2, 1, 1])
    ngram = [0, 3, 0, 4, 0, 2, 3]

    def prepare(slot, r):                       # an empty window, then the conditional prompt's tokens from the offset on
        for b in range(B):
            rwin.load(b)
        rwin.add(slot, P[r][frm[r]:])
    try:
        composed(ctx, "greedy", lambda rt: dict(window=win, dry=dry, no_repeat_ngram=ngram, count_prompt=frm),
                 lambda rt, slot, r: dict(window=rwin, dry=tuple(rows_of(B, slot, x[r], n) for x, n in zip(dry, (0.0, 1.0, 1))),
                                          no_repeat_ngram=rows_of(B, slot, ngram[r], 0)), prepare=prepare)
    finally:
        win.close()
        rwin.close()


def test_composes_with_a_logit_bias_per_request(ctx):
    V = vocab("small")
    rng = np.random.default_rng(5)
    sets = [{int(t): (-np.inf if i % 3 == 0 else float(rng.normal(0, 4))) for i, t in enumerate(rng.choice(V, 40, replace=False))} for _ in range(3)]
    lb = wrk.LogitBias(ctx, V, sets)
    which = [0, 1, 2, wrk.BIAS_NONE, 1, 0, 2]
    try:
        composed(ctx, "greedy", lambda rt: dict(logit_bias=lb, bias_set=which),
                 lambda rt, slot, r: dict(logit_bias=lb, bias_set=rows_of(2, slot, which[r], wrk.BIAS_NONE)))
    finally:
        lb.close()


def test_composes_with_stop_sequences(ctx):
    V = vocab("small")
    free, _ = composed(ctx, "sample", lambda rt: {}, None, replay=False)
    # request 2 ends on the sequence of its draws 2 and 3, request 4 on its first two draws, request 0 on a sequence it never draws
    seqs = [[] for _ in range(R)]
    seqs[2], seqs[4], seqs[0] = [free[2][0][2:4].tolist()], [[V - 1, V - 2], free[4][0][:2].tolist()], [[V - 1, V - 1, V - 1]]
    match = {}

    def each(rt, r, slot, last):
        match[r] = (int(rt.last_stop_match[r]), int(last["match"][slot]))
    got, _ = composed(ctx, "sample", lambda rt: dict(stop_sequences=seqs),
                      lambda rt, slot, r: dict(stop_sequences=rows_of(2, slot, seqs[r], [])), each=each)
    assert [why for _, why, *_ in got][2] == Q.STOP and got[4][1] == Q.STOP and len(got[4][0]) == 2 and got[0][1] == Q.MAX_NEW
    assert match[4] == (1, 1) and match[2][0] == 0 and all(a == b for a, b in match.values())


def test_composes_with_logprobs(ctx):
    rows = {}

    def each(rt, r, slot, last):
        lp, ids, tlp = last["lp"]
        n = last["length"]
        rows[r] = (lp[:n, slot].copy(), ids[:n, slot].copy(), tlp[:n, slot].copy())
    got, qlp = composed(ctx, "sample", lambda rt: dict(logprobs=5), lambda rt, slot, r: dict(logprobs=5), each=each)
    for r in range(R):
        for a, b in zip(qlp[r], rows[r]):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), r
    assert all(len(qlp[r][0]) == MAX_NEW[r] for r in range(R))


def test_init_state_and_negative_init_state_start_the_two_halves(ctx):
    data, V, B = model("small"), vocab("small"), 2
    seed = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2)
    seed.infer(wrk.RnnInput([[(3 + 5 * i) % V for i in range(6)], [(11 + 7 * i) % V for i in range(4)]], 32), mode=1)
    snap, neg_snap = seed.state_read(0), seed.state_read(1)
    seed.close()
    got, _ = composed(ctx, "sample", lambda rt: dict(init_state=snap, negative_init_state=neg_snap), None, init=snap, neg_init=neg_snap)
    cold, _ = composed(ctx, "sample", lambda rt: {}, None, replay=False)
    half, _ = composed(ctx, "sample", lambda rt: dict(init_state=snap), None, replay=False)
    assert any(t.tolist() != u.tolist() for (t, *_), (u, *_) in zip(got, cold))             # the prefixes changed something
    assert any(got[r][0].tolist() != half[r][0].tolist() for r in GUIDED)                   # and so did the partners' alone


# ----------------------------------------------------------------------------------------------------------------- 7. one program
def test_one_program_serves_any_guided_queue(ctx):
    data, V, B, mode = model("small"), vocab("small"), 2, 1
    calls = [dict(requests=prompts(V), negative_prompts=negatives(V), guidance_scale=SCALES, max_new=MAX_NEW, stop=[[]] * R, **pick("sample", R)),
             dict(requests=prompts(V, [2, 4, 1], salt=3), negative_prompts=negatives(V, [3, 0, 1], salt=2), guidance_scale=[0.25, 1.0, 4.0],
                  max_new=[5, 2, 8], stop=[[1, 2], [], [V - 1]], **pick("sample", 3, salt=2)),
             dict(requests=prompts(V, [1, 2, 3, 1, 2, 3, 1, 2, 3], salt=5), negative_prompts=negatives(V, [3, 2, 1, 1, 1, 4, 0, 2, 6], salt=7),
                  guidance_scale=[2.0, 0.0, 1.5, 1.0, 3.0, 0.5, 1.0, 1.25, 2.5], max_new=3, **pick("sample", 9, salt=1))]     # grows the buffers

    def fresh(kw):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
        out = rt.generate_queue_guided(mode=mode, poll_steps=POLL, **kw)
        rt.close()
        return out
    want = [fresh(kw) for kw in calls]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
    got = [rt.generate_queue_guided(mode=mode, poll_steps=POLL, **kw) for kw in calls]
    again = rt.generate_queue_guided(mode=mode, poll_steps=POLL, **calls[0])
    rt.close()
    for (g, grun), (w, wrun) in zip(got + [again], want + [want[0]]):
        assert grun == wrun
        assert plain_rows(g) == plain_rows(w)


# ----------------------------------------------------------------------------------------------------------------- 8. the other loops
@pytest.mark.parametrize("v6", [False, True])
def test_existing_loops_are_unchanged_by_a_guided_queue_call(ctx, v6):
    data, V, B, steps, mode = model("small", v6), vocab("small", v6), 2, 8, 1
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
    zero = zero_state(rt)
    first = [5, 66, 127 % V, 300 % V]
    skw = dict(temperature=[1.0, 0.8, 1.2, 0.9], top_p=[0.9, 1.0, 0.8, 0.95], seed=[11, 12, 13, 14])
    P, N = prompts(V), negatives(V)

    def loops():
        out = []
        for call in (lambda: [rt.generate_greedy(first, steps, mode=mode)[0]],
                     lambda: [rt.generate_sample(first, steps, mode=mode, **skw)[0]],
                     lambda: plain_rows(rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **pick("sample", R))[0]),
                     lambda: list(rt.generate_guided(first[:B], steps, [1.5, 0.5], negative_first_tokens=first[B:], stop=[[], [9]], mode=mode,
                                                     **{k: v[:B] for k, v in skw.items()}))):
            for b in range(2 * B):
                rt.state_load(zero, b)
            out.append([np.array(x).copy() if isinstance(x, np.ndarray) else x for x in call()])
        return out
    before = loops()
    for kind in ("greedy", "sample"):
        rt.generate_queue_guided(P, N, SCALES, max_new=MAX_NEW, mode=mode, **pick(kind, R))
    after = loops()
    rt.close()
    for a, b in zip(before, after):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y


# ----------------------------------------------------------------------------------------------------------------- 9. refusals
@pytest.mark.parametrize("v6", [False, True])
def test_bad_arguments_are_refused_before_any_launch(ctx, v6):
    data, V, B = model("tiny", v6), vocab("tiny", v6), 2
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=2 * B)
    other = wrk.Context(0)
    rt.generate_greedy([3, 4, 5, 6], 5)                             # a state that is not zero
    state = [rt.state_back(b) for b in range(2 * B)]
    good, neg = [[1, 2], [3], [4, 5, 6]], [[7], [8, 9], []]
    size = rt.state_read(0).nbytes
    shared = rt.state_read(1)
    pool = wrk.StatePool(ctx, rt, 2)

    def code(call):
        with pytest.raises(wrk.WrkError) as e:
            call()
        return e.value.code
    bad_calls = [dict(guidance_scale=[1.5, np.nan, 1.0]), dict(guidance_scale=[1.5, np.inf, 1.0]), dict(guidance_scale=[1.5, -0.5, 1.0]),
                 dict(guidance_scale=[1.5, 0.5, 2.0]), dict(guidance_scale=[1.5, 0.5, 0.0]),    # an empty negative prompt with a scale != 1
                 dict(negative_prompts=[[7], [V], []]),                                         # a negative token >= V
                 dict(num_slots=B + 1), dict(num_slots=129),                                    # fewer than 2B state slots; B > 128
                 dict(negative_init_state=wrk.Buffer(ctx, 64)), dict(negative_init_state=wrk.Buffer(ctx, size + 16)),
                 dict(negative_init_state=wrk.Buffer(other, size)), dict(negative_init_state=shared, init_state=shared),
                 dict(requests=[[1], [], [2]]), dict(max_new=[1, 0, 2]), dict(max_steps=0), dict(stop=[[V], [], []])]     # the queue's own
    for kw in bad_calls:
        args = dict(requests=good, negative_prompts=neg, guidance_scale=[1.5, 0.5, 1.0]) | kw
        assert code(lambda: rt.generate_queue_guided(**args)) == wrk.E_ARG, kw
    assert code(lambda: rt.generate_queue_guided(good, neg, [1.5, 0.5, 1.0], mode=1 | (2 << 8))) == wrk.E_UNSUPPORTED       # lanes
    # the old entry points still refuse guidance_scale
    assert code(lambda: rt.generate_queue(good, max_new=2, guidance_scale=1.5)) == wrk.E_UNSUPPORTED
    assert code(lambda: rt.generate_queue(good, max_new=2, guidance_scale=1.5, pool=pool, start_state=0)) == wrk.E_UNSUPPORTED

    # the cases the Python wrapper cannot express, through the C ABI
    fn, mdl = (wrk.hip.wrk_v6_generate_queue_guided, rt.model6) if v6 else (wrk.hip.wrk_v7_generate_queue_guided, rt.model)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    arrays = dict(prompt_tokens=np.array([1, 2, 3, 4], np.uint32), prompt_offsets=np.array([0, 2, 3, 4], np.uint32), max_new=np.array([2, 2, 2], np.uint32))
    garrays = dict(scale=np.array([1.5, 0.5, 1.0], np.float32), negative_tokens=np.array([7, 8, 9], np.uint32),
                   negative_offsets=np.array([0, 1, 3, 3], np.uint32))
    res_arrays = {k: np.zeros(8, np.uint32) for k in ("lengths", "reasons", "slots", "start_steps", "out_tokens", "steps_run")}
    hist = wrk.HistoryPool(ctx, 2, V)

    def call(drop_guide=False, history=False, **over):
        o = wrk.QueueOptions()
        o.num_requests, o.max_steps = 3, 32
        keep = []

        def put(dst, items):
            for k, v in items.items():
                if v is not None:
                    v = np.asarray(v)
                    keep.append(v)
                    setattr(dst, k, v.ctypes.data_as(u32p if v.dtype == np.uint32 else f32p))
        put(o, arrays | {k: v for k, v in over.items() if k in ("guidance_scale",)})
        if history:
            o.history = hist.h
        g = wrk.QueueGuidance()
        put(g, garrays | {k: v for k, v in over.items() if k in garrays})
        res = wrk.QueueResult()
        put(res, res_arrays)
        return fn(ctx.h, mdl, rt.state, B, C.byref(o), C.byref(res), None, 1, None if drop_guide else C.byref(g))
    assert call() == 0                                              # the well-formed call the bad ones are variations of
    for b in range(2 * B):
        rt.state_load(state[b], b)
    bad = [call(drop_guide=True), call(scale=None), call(negative_offsets=None), call(negative_tokens=None),
           call(negative_offsets=np.array([1, 1, 3, 3], np.uint32)), call(negative_offsets=np.array([0, 2, 1, 3], np.uint32)),
           call(guidance_scale=np.ones(3, np.float32)),             # the scales come from `guide`
           call(history=True)]                                      # no entry point takes a pool and guidance
    assert bad == [wrk.E_ARG] * len(bad), bad
    for b in range(2 * B):
        assert np.array_equal(bits(rt.state_back(b)), bits(state[b])), b
    hist.close()
    pool.close()
    other.close()
    rt.close()
