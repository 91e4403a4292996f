"""The request queue of the decode loops (web-rwkv-gguf_amd/csrc/wrk_queue.hip) through `Runtime.generate_queue`, against
the restatement in tests/queue_ref.py and against a replay of every request on its own.

The replay of a request runs it alone in the slot the queue gave it, with filler tokens in the other slots: n - 1 one-step calls of the
same pick kind feed the prompt (their draws are discarded; with penalties the occurrence row is reset afterwards), then `generate_stop`
runs from p_{n-1} with the request's parameters, stop set and steps = max_new.  Reply tokens and length must be equal; slot, start_step
and reason must be those of queue_ref's schedule computed from the observed lengths, and steps_run must be queue_ref.steps_run of them:
the host waits for block k's live count before it submits block k + 2, so exactly one block follows the one in which the last request
ends (min(max_steps, (ceil(needed / poll) + 1) * poll)); the looser bound (ceil(needed / poll) + 2) * poll is asserted beside it.
The replay runtime is one per test; every slot of it (and of its occurrence table) is set to what a fresh runtime holds before each replay.

Shapes: R = 7 requests, prompts of 1 to 5 tokens, max_new <= 12, B in {1, 2, 4}: the batch-1 engine, two slots ending in the same step
(requests 0 and 1 end in step 5 by max_new), idle slots at the end, and a slot serving three and more requests in a row.  The stop ids
come from what the same queue draws without stops (a token that does not occur earlier in the reply), so ends are forced where intended."""
import ctypes as C
import functools

import numpy as np
import pytest

import queue_ref as Q
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

PROMPT_LENS = [3, 1, 5, 2, 4, 1, 2]
MAX_NEW = [4, 6, 12, 5, 9, 1, 7]
R = len(PROMPT_LENS)
POLL = 4


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model(cfg="small", v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS[cfg], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS[cfg], 42)


def vocab(cfg="small", v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)[cfg].num_vocab


def prompts(V, lens=PROMPT_LENS, salt=0):
    return [[(7 + salt + 13 * r + 29 * i) % V for i in range(n)] for r, n in enumerate(lens)]


def pick(kind, n, salt=0):
    """per-request parameters of the pick kind, all different"""
    if kind == "greedy":
        return {}
    kw = dict(temperature=[[1.0, 0.8, 1.2, 0.9][(r + salt) % 4] for r in range(n)], top_p=[[0.9, 1.0, 0.8, 0.95][(r + salt) % 4] for r in range(n)],
              seed=[11 + salt + r for r in range(n)])
    if kind == "pen":
        kw |= dict(presence=[0.1 + 0.05 * r for r in range(n)], frequency=[0.3 - 0.02 * r for r in range(n)],
                   decay=[1.0 if r == 3 else 0.99 + 0.001 * r for r in range(n)])
    return kw


def one(kw, r):
    return {k: v[r] for k, v in kw.items()}


def zero_state(rt):
    L, D, S = rt.info.num_layer, rt.info.num_emb, rt.info.num_emb // rt.info.num_head
    return np.zeros((L, S + 2, D), np.float32)


class Replayer:
    """Replays one request alone in a slot of a runtime whose every slot holds what a fresh runtime holds."""

    def __init__(self, ctx, data, V, B, kind, mode, ban=None, init=None):
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        self.occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
        self.V, self.B, self.kind, self.mode, self.ban, self.init = V, B, kind, mode, ban or {}, init
        self.zero = zero_state(self.rt)

    def reset_row(self, b):
        self.occ.load(b)
        if b in self.ban:
            self.occ.ban(b, self.ban[b])

    def step(self, first, kw):
        if self.kind == "greedy":
            self.rt.generate_greedy(first, 1, mode=self.mode)
        elif self.kind == "sample":
            self.rt.generate_sample(first, 1, mode=self.mode, **kw)
        else:
            self.rt.generate_penalized(first, 1, self.occ, mode=self.mode, **kw)

    def __call__(self, slot, prompt, stop, max_new, kw):
        rt, B = self.rt, self.B
        for b in range(B):
            rt.state_load(self.zero, b)
            if self.occ:
                self.reset_row(b)
        if self.init is not None:
            rt.state_write(self.init, slot)
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
        tok, lens = rt.generate_stop(first, max_new, stops, mode=self.mode, **kw, **pk)
        return tok[:lens[slot], slot].copy()

    def close(self):
        if self.occ:
            self.occ.close()
        self.rt.close()


def new_at(reply, k):
    """(index j >= k, id): the first token of the reply at or after index k that does not occur earlier in it"""
    col = [int(t) for t in reply]
    for j in range(k, len(col)):
        if col[j] not in col[:j]:
            return j, col[j]
    raise AssertionError(f"the reply draws no new token from index {k} on: {col}")


def forced_stops(plain, V):
    """requests 0, 1, 3 and 5 end by max_new (0 and 1 in the same step); 2 and 4 end mid-reply on the second of two stop ids; 6 ends on y_0"""
    spare = next(i for i in range(V - 1, -1, -1) if all(i not in set(t.tolist()) for t, *_ in plain))
    stops = [[] for _ in range(R)]
    stops[2] = [spare, new_at(plain[2][0], 3)[1]]
    stops[4] = [new_at(plain[4][0], 2)[1]]
    stops[6] = [int(plain[6][0][0])]
    return stops


def check_against_replays(got, steps_run, rep, P, stops, max_new, kw, B, max_steps):
    replies = [rep(got[r][2], P[r], stops[r], max_new[r], one(kw, r)) for r in range(len(P))]
    want, needed = Q.run(P, replies, stops, max_new, B)
    for r in range(len(P)):
        t, why, slot, start = got[r]
        print(f"request {r}: slot {slot} start {start} reason {why} reply {t.tolist()} replay {replies[r].tolist()}")
        assert t.tolist() == replies[r].tolist(), f"request {r}"
        assert (why, slot, start) == want[r][1:], f"request {r}: {(why, slot, start)} against the schedule {want[r][1:]}"
    print(f"steps_run {steps_run}, needed {needed}, bound {Q.steps_run_bound(needed, POLL, max_steps)}")
    assert steps_run == Q.steps_run(needed, POLL, max_steps)
    assert needed <= steps_run <= Q.steps_run_bound(needed, POLL, max_steps)
    return replies, needed


def replay_identity(ctx, kind, mode, v6, B):
    data, V = model("small", v6), vocab("small", v6)
    P, kw = prompts(V), pick(kind, R)
    max_steps = sum(PROMPT_LENS) + sum(MAX_NEW)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        rt.generate_greedy([5] * B, 3, mode=mode)                  # the call does not continue from what the slots held
        plain, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        assert [len(t) for t, *_ in plain] == MAX_NEW and [why for _, why, *_ in plain] == [Q.MAX_NEW] * R
        stops = forced_stops(plain, V)
        got, run = rt.generate_queue(P, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        replies, _ = check_against_replays(got, run, rep, P, stops, MAX_NEW, kw, B, max_steps)
        # what the shapes are there for
        assert [why for _, why, *_ in got] == [Q.MAX_NEW, Q.MAX_NEW, Q.STOP, Q.MAX_NEW, Q.STOP, Q.MAX_NEW, Q.STOP]
        assert len(got[2][0]) >= 4 and len(got[4][0]) >= 3 and len(got[6][0]) == 1
        if B >= 2:
            assert got[0][3] + PROMPT_LENS[0] + len(got[0][0]) == got[1][3] + PROMPT_LENS[1] + len(got[1][0])      # the same-step tie
            assert (got[B][2], got[B + 1][2]) == (0, 1) and got[B][3] == got[B + 1][3]
        if B <= 2:
            assert max(sum(1 for g in got if g[2] == b) for b in range(B)) >= 3
    finally:
        rep.close()
        if occ:
            occ.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 1. replay identity
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("mode,v6", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("kind", ["greedy", "sample", "pen"])
def test_replay_identity(ctx, kind, mode, v6, B):
    replay_identity(ctx, kind, mode, v6, B)


def test_replay_identity_eager(ctx, monkeypatch):
    monkeypatch.setenv("WRK_NO_GRAPH", "1")
    replay_identity(ctx, "pen", 1, False, 2)


def test_replay_identity_engine_off(ctx, monkeypatch):
    monkeypatch.setenv("WRK_ENGINE", "0")
    replay_identity(ctx, "sample", 1, False, 1)


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("mode,v6", [(0, False), (1, False), (1, True)])
def test_a_slot_does_not_depend_on_its_neighbours(ctx, mode, v6, B):
    """What the replay rests on: the same sequence in the same slot under two neighbour sets gives the same logits bits."""
    data, V, steps = model("small", v6), vocab("small", v6), 6
    out = []
    for salt in (0, 1):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        first = [(40 + 7 * b + 101 * salt) % V for b in range(B)]
        first[B - 1] = 9
        tok, _, logits = rt.generate_greedy(first, steps, mode=mode, want_logits=True)
        out.append((tok[:, B - 1].copy(), bits(logits[B - 1]).copy(), bits(rt.state_back(B - 1)).copy()))
        rt.close()
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


# ----------------------------------------------------------------------------------------------------------------- 2. reset, bans
def test_reset_is_complete_and_bans_stay(ctx):
    data, V, B, kind, mode = model("small"), vocab("small"), 2, "pen", 1
    P, kw = prompts(V), pick(kind, R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V)
    plain, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, occurrence=occ, **kw)
    # ban, per slot, the token its requests drew most often: every later request of the slot must do without it
    ban = {}
    for b in range(B):
        drawn = np.concatenate([t for t, _, slot, _ in plain if slot == b])
        ids, n = np.unique(drawn, return_counts=True)
        ban[b] = [int(ids[n.argmax()])]
        occ.ban(b, ban[b])
    rep = Replayer(ctx, data, V, B, kind, mode, ban=ban)
    try:
        got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, occurrence=occ, **kw)
        stops = [[] for _ in range(R)]
        check_against_replays(got, run, rep, P, stops, MAX_NEW, kw, B, sum(PROMPT_LENS) + sum(MAX_NEW))
        for t, _, slot, _ in got:
            assert ban[slot][0] not in t.tolist()
        assert any(t.tolist() != u.tolist() for (t, *_), (u, *_) in zip(got, plain))        # the bans changed something
        for b in range(B):
            assert (occ.back(b)[1][ban[b][0]] & 2) == 2
    finally:
        rep.close()
        occ.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 3. init_state
@pytest.mark.parametrize("v6", [False, True])
def test_init_state_is_the_start_of_every_request(ctx, v6):
    data, V, B, kind, mode = model("small", v6), vocab("small", v6), 2, "sample", 1
    P, kw = prompts(V), pick(kind, R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    prefix = [(3 + 5 * i) % V for i in range(6)]
    rt.infer(wrk.RnnInput([prefix] * B, 32), mode=1)
    snap = rt.state_read(0)
    rep = Replayer(ctx, data, V, B, kind, mode, init=snap)
    try:
        stops = [[] for _ in range(R)]
        got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, init_state=snap, **kw)
        check_against_replays(got, run, rep, P, stops, MAX_NEW, kw, B, sum(PROMPT_LENS) + sum(MAX_NEW))
        cold, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw)
        assert any(t.tolist() != u.tolist() for (t, *_), (u, *_) in zip(got, cold))         # the prefix changed something
    finally:
        rep.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 4. one program
def test_one_program_serves_any_queue(ctx):
    data, V, B, mode = model("small"), vocab("small"), 2, 1
    calls = [dict(requests=prompts(V), max_new=MAX_NEW, stop=[[]] * R, **pick("sample", R)),
             dict(requests=prompts(V, [2, 4, 1], salt=3), max_new=[5, 2, 8], stop=[[1, 2], [], [V - 1]], **pick("sample", 3, salt=2)),
             dict(requests=prompts(V, [1, 2, 3, 1, 2, 3, 1, 2, 3], salt=5), max_new=3, **pick("sample", 9, salt=1))]     # grows the buffers

    def fresh(kw):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        out = rt.generate_queue(mode=mode, poll_steps=POLL, **kw)
        rt.close()
        return out
    want = [fresh(kw) for kw in calls]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    zero = zero_state(rt)
    first = [5, 66]
    before, _ = rt.generate_sample(first, 8, mode=mode, seed=[3, 4])
    got = [rt.generate_queue(mode=mode, poll_steps=POLL, **kw) for kw in calls]
    for b in range(B):
        rt.state_load(zero, b)
    after, _ = rt.generate_sample(first, 8, mode=mode, seed=[3, 4])
    rt.close()
    for (g, grun), (w, wrun) in zip(got, want):
        assert grun == wrun
        assert [(t.tolist(), a, b, c) for t, a, b, c in g] == [(t.tolist(), a, b, c) for t, a, b, c in w]
    assert np.array_equal(before, after)


# ----------------------------------------------------------------------------------------------------------------- 5. early exit, cap
def test_early_exit_and_cap(ctx):
    data, V, B, mode, poll = model("small"), vocab("small"), 2, 1, 8
    P, kw = prompts(V), pick("sample", R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    full, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=poll, max_steps=2048, **kw)
    stops = [[] for _ in range(R)]
    replies = [t for t, *_ in full]
    want, needed = Q.run(P, replies, stops, MAX_NEW, B)
    print(f"early exit: steps_run {run}, needed {needed}, bound {Q.steps_run_bound(needed, poll, 2048)}")
    assert run == Q.steps_run(needed, poll, 2048) == (-(-needed // poll) + 1) * poll
    assert needed <= run <= Q.steps_run_bound(needed, poll, 2048) == (-(-needed // poll) + 2) * poll
    assert [(t.tolist(), a, b, c) for t, a, b, c in full] == [(t.tolist(), a, b, c) for t, a, b, c in want]
    # caps: one that cuts requests mid-reply and leaves later ones undispatched, one that ends on a request's last step, one step
    last_start = max(c for *_, c in full)
    for cap in (needed - 2, last_start, last_start - 1, 7, 1):
        got, crun = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=poll, max_steps=cap, **kw)
        cut, _ = Q.run(P, replies, stops, MAX_NEW, B, max_steps=cap)
        print(f"cap {cap}: reasons {[a for _, a, *_ in got]} lengths {[len(t) for t, *_ in got]}")
        assert crun == cap
        assert [(t.tolist(), a, b, c) for t, a, b, c in got] == [(t.tolist(), a, b, c) for t, a, b, c in cut], cap
    reasons = [a for _, a, *_ in Q.run(P, replies, stops, MAX_NEW, B, max_steps=7)[0]]
    assert Q.CAP in reasons and Q.NEVER in reasons and Q.MAX_NEW in reasons
    rt.close()


# ----------------------------------------------------------------------------------------------------------------- 6. the other loops
@pytest.mark.parametrize("v6", [False, True])
def test_existing_loops_are_unchanged_by_a_queue_call(ctx, v6):
    data, V, B, steps, mode = model("small", v6), vocab("small", v6), 3, 10, 1
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V)
    zero = zero_state(rt)
    first = [5, 66, 127 % V]
    skw = dict(temperature=[1.0, 0.8, 1.2], top_p=[0.9, 1.0, 0.8], seed=[11, 12, 13])
    pkw = dict(presence=0.3, frequency=0.2, decay=0.996)

    def loops():
        out = []
        for call in (lambda: rt.generate_greedy(first, steps, mode=mode)[0],
                     lambda: rt.generate_sample(first, steps, mode=mode, **skw)[0],
                     lambda: rt.generate_penalized(first, steps, occ, mode=mode, **skw, **pkw)[0],
                     lambda: rt.generate_stop(first, steps, [[], [9], []], mode=mode, occurrence=occ, **skw, **pkw)[0]):
            for b in range(B):
                rt.state_load(zero, b)
                occ.load(b)
            out.append(call().copy())
        return out
    before = loops()
    for kind in ("greedy", "sample", "pen"):
        rt.generate_queue(prompts(V), max_new=MAX_NEW, mode=mode, **pick(kind, R), **(dict(occurrence=occ) if kind == "pen" else {}))
    after = loops()
    occ.close()
    rt.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


# ----------------------------------------------------------------------------------------------------------------- 7. one dispatch rule
@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("family", ["mirostat", "filtered"])
def test_host_and_device_dispatch_agree(ctx, v6, family):
    """The same five requests in order and in reversed order on two slots: the requests that the host dispatched at step 0 of one call
    are dispatched by a refill on the device in the other, and the other way round.  With every feature on that a dispatch writes --
    penalties, a token window with DRY, a grammar whose state a reply moves, stop ids and stop sequences, prompt intake -- a request's
    reply, reason, final mu, final automaton state and match word are equal bit for bit: "a reply does not depend on the slot or the
    step".  Whether each reply is the right one is the business of the replays in the dry / grammar / mirostat / stopseq / history files."""
    V, B, n = vocab("small", v6), 2, 5
    lens, max_new = [3, 1, 2, 1, 3], [6, 4, 5, 6, 3]
    P = prompts(V, lens)
    per = pick("pen", n) | dict(grammar_state=[r % 2 for r in range(n)], no_repeat_ngram=[0, 3, 0, 4, 0], count_prompt=[0, 1, 0, 0, 2])
    if family == "mirostat":
        tau = [3.0, 2.5, 4.0, 3.5, 2.0]
        per |= dict(mirostat_mu=[2 * t + 0.25 * r for r, t in enumerate(tau)])
        family_kw = lambda order: dict(mirostat=([tau[r] for r in order], [0.1 + 0.05 * r for r in order]))
    else:
        per |= dict(top_k=[40, 5, 200, 17, 3], min_p=[0.0, 0.02, 0.0, 0.01, 0.05])
        family_kw = lambda order: {}
    dry = ([3.0, 0.0, 25.0, 40.0, 3.0], [1.75, 1.75, 2.0, 1.75, 1e30], [1, 2, 1, 1, 2])
    rt = wrk.Runtime(ctx, wrk.GgufReader(model("small", v6)), num_batch=B)
    occ, win = wrk.Occurrence(ctx, B, V), wrk.TokenWindow(ctx, B, V, 8)
    # two states, every token allowed: an odd token id toggles the state, so the final state depends on the whole reply
    gram = wrk.Grammar(ctx, V, np.arange(V) % 2, [[0, 1], [1, 0]])

    def call(order, stop, seqs):
        for b in range(B):
            occ.load(b)
            win.load(b)
        kw = {k: [v[r] for r in order] for k, v in per.items()} | family_kw(order)
        res, _ = rt.generate_queue([P[r] for r in order], stop=[stop[r] for r in order], max_new=[max_new[r] for r in order], mode=1, poll_steps=POLL,
                                   occurrence=occ, window=win, dry=tuple([x[r] for r in order] for x in dry), grammar=gram,
                                   stop_sequences=None if seqs is None else [seqs[r] for r in order], **kw)
        mu, gs, match = rt.last_mirostat_mu, rt.last_grammar_state, rt.last_stop_match
        at = {r: i for i, r in enumerate(order)}
        return [dict(tok=res[at[r]][0].tolist(), reason=res[at[r]][1], start=res[at[r]][3], mu=None if mu is None else int(bits(mu[at[r]])),
                     gs=int(gs[at[r]]), match=None if match is None else int(match[at[r]])) for r in range(n)]
    try:
        plain = call(list(range(n)), [[]] * n, None)
        assert all(len(p["tok"]) == m for p, m in zip(plain, max_new))
        # request 0 ends on the id of its third draw, request 4 on the stop sequence of its first two draws
        stop, seqs = [[] for _ in range(n)], [[] for _ in range(n)]
        stop[0], seqs[4] = [plain[0]["tok"][2]], [plain[4]["tok"][:2]]
        fwd, rev = call(list(range(n)), stop, seqs), call(list(range(n))[::-1], stop, seqs)
    finally:
        gram.close()
        win.close()
        occ.close()
        rt.close()
    assert fwd[0]["reason"] == Q.STOP and fwd[4]["reason"] == Q.STOP and fwd[4]["match"] == 0 and len(fwd[4]["tok"]) == 2
    assert len({tuple(p["tok"]) for p in fwd}) > 1                      # the requests do not all draw the same reply
    for r in range(n):
        host_first = r < B              # dispatched by the host at step 0 in order, by the device in reversed order -- or the reverse
        assert (fwd[r]["start"] == 0) == host_first and (rev[r]["start"] == 0) == (n - 1 - r < B), (r, fwd[r], rev[r])
        assert {k: v for k, v in fwd[r].items() if k != "start"} == {k: v for k, v in rev[r].items() if k != "start"}, (r, fwd[r], rev[r])


# ----------------------------------------------------------------------------------------------------------------- 8. validation
@pytest.mark.parametrize("v6", [False, True])
def test_bad_arguments_are_rejected_before_any_launch(ctx, v6):
    data, V, B = model("tiny", v6), vocab("tiny", v6), 2
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ, occ1, occv = wrk.Occurrence(ctx, B, V), wrk.Occurrence(ctx, 1, V), wrk.Occurrence(ctx, B, V + 4)
    other = wrk.Context(0)
    occ_other = wrk.Occurrence(other, B, V)
    rt.generate_greedy([3, 4], 5)                                   # a state that is not zero
    state = [rt.state_back(b) for b in range(B)]
    good = [[1, 2], [3], [4, 5, 6]]
    bad_calls = [dict(requests=[]), dict(requests=[[1], []]), dict(requests=good, max_new=[1, 0, 2]), dict(requests=[[1], [V]]),
                 dict(requests=good, stop=[[V], [], []]), dict(requests=good, stop=[list(range(wrk.MAX_STOP_TOKENS + 1)), [], []]),
                 dict(requests=good, max_steps=0), dict(requests=good, temperature=-1.0), dict(requests=good, occurrence=occ, decay=1.5),
                 dict(requests=good, occurrence=occ1), dict(requests=good, occurrence=occv), dict(requests=good, occurrence=occ_other),
                 dict(requests=good, init_state=wrk.Buffer(ctx, 64)), dict(requests=good, init_state=wrk.Buffer(ctx, rt.state_read(0).nbytes + 16))]
    for kw in bad_calls:
        with pytest.raises(wrk.WrkError) as e:
            rt.generate_queue(**kw)
        assert e.value.code == wrk.E_ARG, kw
    with pytest.raises(wrk.WrkError) as e:
        rt.generate_queue(good, mode=1 | (2 << 8))                  # lanes
    assert e.value.code == wrk.E_UNSUPPORTED

    # the cases the Python wrapper cannot express, through the C ABI
    fn, mdl = (wrk.hip.wrk_v6_generate_queue, rt.model6) if v6 else (wrk.hip.wrk_v7_generate_queue, rt.model)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    arrays = dict(prompt_tokens=np.array([1, 2, 3, 4], np.uint32), prompt_offsets=np.array([0, 2, 3, 4], np.uint32),
                  max_new=np.array([2, 2, 2], np.uint32), stop_tokens=np.array([1, 2, 3], np.uint32),
                  stop_offsets=np.array([0, 1, 1, 3], np.uint32))
    t, sd = np.ones(3, np.float32), np.zeros(3, np.uint32)
    res_arrays = {k: np.zeros(8, np.uint32) for k in ("lengths", "reasons", "slots", "start_steps", "out_tokens", "steps_run")}

    def call(drop_opt=False, drop_out=False, drop_result=None, num_requests=3, **over):
        o = wrk.QueueOptions()
        o.num_requests, o.max_steps = num_requests, 32
        keep = []
        for k, v in (arrays | over).items():
            if v is not None:
                v = np.asarray(v)
                keep.append(v)
                setattr(o, k, v.ctypes.data_as(u32p if v.dtype == np.uint32 else f32p))
        res = wrk.QueueResult()
        for k, v in res_arrays.items():
            if k != drop_result:
                setattr(res, k, v.ctypes.data_as(u32p))
        return fn(ctx.h, mdl, rt.state, B, None if drop_opt else C.byref(o), None if drop_out else C.byref(res), None, 1)
    assert call() == 0                                              # the well-formed call the bad ones are variations of
    for b in range(B):
        rt.state_load(state[b], b)
    bad = [call(drop_opt=True), call(drop_out=True), call(drop_result="lengths"), call(drop_result="steps_run"), call(num_requests=0),
           call(prompt_tokens=None), call(prompt_offsets=None), call(max_new=None),
           call(prompt_offsets=np.array([1, 2, 3, 4], np.uint32)), call(prompt_offsets=np.array([0, 3, 2, 4], np.uint32)),
           call(prompt_offsets=np.array([0, 2, 2, 4], np.uint32)),                       # an empty prompt
           call(stop_offsets=np.array([1, 1, 2, 3], np.uint32)), call(stop_offsets=np.array([0, 2, 1, 3], np.uint32)),
           call(stop_offsets=None), call(temperature=t), call(temperature=t, top_p=t), call(top_p=t, seed=sd), call(presence=t)]
    assert bad == [wrk.E_ARG] * len(bad), bad
    for b in range(B):
        assert np.array_equal(bits(rt.state_back(b)), bits(state[b])), b
    for o in (occ, occ1, occv, occ_other):
        o.close()
    other.close()
    rt.close()
