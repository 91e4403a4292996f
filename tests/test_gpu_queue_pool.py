"""The state pool of the request queue (web-rwkv-gguf_amd/csrc/wrk_queue.hip) through `Runtime.generate_queue(pool=...)`,
against the restatements in tests/queue_pool_ref.py and tests/queue_ref.py and against a replay of every request on its own.

The replay of a request runs it alone in the slot the queue gave it, from the start state the request named (what the entry held BEFORE
the call; zeros without one), with filler tokens in the other slots: n - 1 one-step calls of the same pick kind feed the prompt, then
`generate_stop` runs from p_{n-1} with the request's parameters, stop set and steps = max_new.  The reply must be equal and the entry the
request saves to must be bit-equal to the replay's `state_back(slot)`: `generate_stop` freezes a sequence's state at the step that ends
it -- the last reply token drawn, not fed -- which is the state the contract saves.  Every entry that no finished request saves to must
keep its bits; slot, start step, reason and steps_run must be queue_ref's.

Shapes: tests/test_gpu_queue.py's -- synth "small", R = 7 requests, prompts of 1 to 5 tokens, max_new <= 12, B in {1, 2, 4}.  The pool has
6 entries: 0, 1, 2 hold the states of three prefixes, 3, 4, 5 hold random bit patterns (NaN patterns among them: entries are moved, never
computed with).  Requests 1 and 2 share entry 0 read-only, 3 and 4 are sessions in place (entries 1 and 2), 2 saves to entry 4 and the
last request, 6, from a cold start to entry 3; entry 5 is named by nobody."""
import ctypes as C
import functools

import numpy as np
import pytest

import queue_pool_ref as PR
import queue_ref as Q
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

PROMPT_LENS = [3, 1, 5, 2, 4, 1, 2]
MAX_NEW = [4, 6, 12, 5, 9, 1, 7]
R = len(PROMPT_LENS)
POLL = 4
ENTRIES = 6
START = [None, 0, 0, 1, 2, None, None]
SAVE = [None, None, 4, 1, 2, None, 3]
MAX_STEPS = sum(PROMPT_LENS) + sum(MAX_NEW)


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


def pattern(rt, seed):
    """random bits in a state's shape, NaN and infinity patterns among them"""
    shape = zero_state(rt).shape
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint32).view(np.float32)


def filled_pool(ctx, rt, V, entries=ENTRIES, salt=0):
    """entries 0, 1, 2: the states `infer` leaves after three different prefixes; the others: bit patterns.  Returns the pool, what every
    entry holds on the host and a device snapshot of each."""
    pool = wrk.StatePool(ctx, rt, entries)
    zero = zero_state(rt)
    for k in range(entries):
        if k < 3:
            prefix = [(3 + salt + 5 * i + 11 * k) % V for i in range(4 + 2 * k)]
            rt.state_load(zero, 0)                                 # `infer` continues from what the slot holds
            rt.infer(wrk.RnnInput([prefix] * rt.num_batch, 32), mode=1)
            pool.put(k, rt.state_read(0))
        else:
            pool.load(k, pattern(rt, 100 + salt + k))
    before = [pool.back(k) for k in range(entries)]
    assert not any(np.array_equal(bits(before[a]), bits(before[b])) for a in range(entries) for b in range(a))
    return pool, before, [pool.get(k) for k in range(entries)]


class Replayer:
    """Replays one request alone in a slot of a runtime whose every other slot holds what a fresh runtime holds."""

    def __init__(self, ctx, data, V, B, kind, mode):
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        self.occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
        self.V, self.B, self.kind, self.mode = V, B, kind, mode
        self.zero = zero_state(self.rt)

    def step(self, first, kw):
        if self.kind == "greedy":
            self.rt.generate_greedy(first, 1, mode=self.mode)
        elif self.kind == "sample":
            self.rt.generate_sample(first, 1, mode=self.mode, **kw)
        else:
            self.rt.generate_penalized(first, 1, self.occ, mode=self.mode, **kw)

    def begin(self, slot, snapshot):
        for b in range(self.B):
            self.rt.state_load(self.zero, b)
            if self.occ:
                self.occ.load(b)
        if snapshot is not None:
            self.rt.state_write(snapshot, slot)

    def turn(self, slot, prompt, stop, max_new, kw):
        """feeds `prompt` and draws the reply, continuing from what the slot holds; returns (reply, the slot's frozen state)"""
        rt, B = self.rt, self.B
        first = [(3 + 17 * b) % self.V for b in range(B)]
        for t in prompt[:-1]:
            first[slot] = t
            self.step(first, kw)
        if self.occ:
            self.occ.load(slot)
        first[slot] = prompt[-1]
        stops = [[] for _ in range(B)]
        stops[slot] = list(stop)
        pk = dict(occurrence=self.occ) if self.occ else {}
        tok, lens = rt.generate_stop(first, max_new, stops, mode=self.mode, **kw, **pk)
        return tok[:lens[slot], slot].copy(), rt.state_back(slot)

    def __call__(self, slot, snapshot, prompt, stop, max_new, kw):
        self.begin(slot, snapshot)
        return self.turn(slot, prompt, stop, max_new, kw)

    def close(self):
        if self.occ:
            self.occ.close()
        self.rt.close()


def first_new(reply, k):
    """the first token of the reply at or after index k that does not occur earlier in it (else the first such before k: index 0 at worst)"""
    col = [int(t) for t in reply]
    for j in list(range(k, len(col))) + list(range(k - 1, -1, -1)):
        if col[j] not in col[:j]:
            return col[j]


def forced_stops(plain, V):
    """requests 2 and 4 end mid-reply on the second of two stop ids where their replies allow it, 6 ends on y_0; the others by max_new"""
    spare = next(i for i in range(V - 1, -1, -1) if all(i not in set(t.tolist()) for t, *_ in plain))
    stops = [[] for _ in range(R)]
    stops[2] = [spare, first_new(plain[2][0], 3)]
    stops[4] = [first_new(plain[4][0], 2)]
    stops[6] = [int(plain[6][0][0])]
    return stops


def check_pool_call(got, steps_run, saved, rep, P, stops, max_new, kw, B, max_steps, start, save, pool, before, snaps):
    """replies, schedule, saved flags and every pool entry against the replays and the two restatements"""
    n = len(P)
    PR.validate(start, save, pool.entries)
    replays = [rep(got[r][2], None if start[r] is None else snaps[start[r]], P[r], stops[r], max_new[r], one(kw, r)) for r in range(n)]
    replies = [t for t, _ in replays]
    want, needed = Q.run(P, replies, stops, max_new, B)
    for r in range(n):
        t, why, slot, step = got[r]
        print(f"request {r}: slot {slot} start {step} reason {why} reply {t.tolist()} replay {replies[r].tolist()}")
        assert t.tolist() == replies[r].tolist(), f"request {r}"
        assert (why, slot, step) == want[r][1:], f"request {r}: {(why, slot, step)} against the schedule {want[r][1:]}"
    print(f"steps_run {steps_run}, needed {needed}")
    assert steps_run == Q.steps_run(needed, POLL, max_steps)
    reasons = [why for _, why, *_ in got]
    assert saved == PR.saved(save, reasons)
    written = PR.written(save, reasons)
    for k in range(pool.entries):
        have = bits(pool.back(k))
        if k in written:
            assert np.array_equal(have, bits(replays[written[k]][1])), f"entry {k}: not the final state of request {written[k]}"
            assert not np.array_equal(have, bits(before[k])), f"entry {k} was not written"
        else:
            assert np.array_equal(have, bits(before[k])), f"entry {k} is named by no finished request and changed"
    return replies


def last_of_slot(got):
    """the requests that are the last ones their slots serve"""
    return {max(r for r, g in enumerate(got) if g[2] == b) for b in {g[2] for g in got}}


def replay_identity(ctx, kind, mode, v6, B):
    data, V = model("small", v6), vocab("small", v6)
    P, kw = prompts(V), pick(kind, R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
    pk = dict(occurrence=occ) if occ else {}
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        pool, before, snaps = filled_pool(ctx, rt, V)
        # reading alone: the stop ids are chosen from what the same requests draw from the same start states without stops
        plain, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, start_state=START, **kw, **pk)
        assert rt.last_queue_saved == [False] * R
        assert all(np.array_equal(bits(pool.back(k)), bits(before[k])) for k in range(ENTRIES))
        stops = forced_stops(plain, V)
        got, run = rt.generate_queue(P, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, start_state=START,
                                     save_state=SAVE, **kw, **pk)
        check_pool_call(got, run, rt.last_queue_saved, rep, P, stops, MAX_NEW, kw, B, MAX_STEPS, START, SAVE, pool, before, snaps)
        # what the shapes are there for
        reasons = [why for _, why, *_ in got]
        assert reasons[6] == Q.STOP and reasons.count(Q.STOP) >= 2 and reasons.count(Q.MAX_NEW) >= 3 and set(reasons) == {Q.STOP, Q.MAX_NEW}
        assert rt.last_queue_saved == [k is not None for k in SAVE]
        end = [g[3] + PROMPT_LENS[r] - 1 + len(g[0]) - 1 for r, g in enumerate(got)]        # the step that ends request r
        # a slot that ends and restarts in one step, saving to one entry while its next request starts from another
        both = [(r, q) for r in range(R) for q in range(R) if got[q][2] == got[r][2] and got[q][3] == end[r] + 1
                and SAVE[r] is not None and START[q] is not None and START[q] != SAVE[r]]
        # a saved request after which its slot goes idle
        idle = [r for r in last_of_slot(got) if SAVE[r] is not None]
        print(f"B = {B}: save-and-restart transitions {both}, saved last requests {idle}")
        assert idle
        if B == 1:
            assert (2, 3) in both and (3, 4) in both and idle == [6]
        # the start states changed something: the same requests from zeros draw other replies
        cold, _ = rt.generate_queue(P, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw, **pk)
        assert rt.last_queue_saved is None
        assert any(t.tolist() != u.tolist() for (t, *_), (u, *_) in zip(got, cold))
        pool.close()
    finally:
        rep.close()
        if occ:
            occ.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 2. replay identity
@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("mode,v6", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("kind", ["greedy", "sample"])
def test_saved_states_and_replies_equal_replays(ctx, kind, mode, v6, B):
    replay_identity(ctx, kind, mode, v6, B)


def test_saved_states_and_replies_equal_replays_penalised(ctx):
    replay_identity(ctx, "pen", 1, False, 2)


# ----------------------------------------------------------------------------------------------------------------- 7. eager, engine off
def test_replay_identity_eager(ctx, monkeypatch):
    monkeypatch.setenv("WRK_NO_GRAPH", "1")
    replay_identity(ctx, "pen", 1, False, 2)


def test_replay_identity_engine_off(ctx, monkeypatch):
    monkeypatch.setenv("WRK_ENGINE", "0")
    replay_identity(ctx, "sample", 1, False, 1)


# ----------------------------------------------------------------------------------------------------------------- 3. a session
@pytest.mark.parametrize("v6", [False, True])
def test_a_session_across_calls(ctx, v6):
    """Two rounds of four conversations on two slots, each conversation in place on its own entry.  The lengths keep every conversation
    in the same slot in both rounds, so the reference -- one runtime that never touches the state between the turns -- runs it there."""
    data, V, B, mode, n = model("small", v6), vocab("small", v6), 2, 1, 4
    kw = pick("sample", n)
    P1, M1 = prompts(V, [2, 4, 3, 2]), [3, 6, 4, 5]
    tail, M2 = prompts(V, [2, 4, 1, 2], salt=9), [2, 7, 8, 3]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    rep = Replayer(ctx, data, V, B, "sample", mode)
    try:
        pool = wrk.StatePool(ctx, rt, n)
        own = list(range(n))
        r1, _ = rt.generate_queue(P1, max_new=M1, mode=mode, poll_steps=POLL, pool=pool, start_state=own, save_state=own, **kw)
        assert rt.last_queue_saved == [True] * n
        # the last reply token was drawn, not fed: it opens the next turn
        P2 = [[int(r1[r][0][-1])] + tail[r] for r in range(n)]
        r2, _ = rt.generate_queue(P2, max_new=M2, mode=mode, poll_steps=POLL, pool=pool, start_state=own, save_state=own, **kw)
        assert rt.last_queue_saved == [True] * n
        assert [g[2] for g in r1] == [g[2] for g in r2] == [0, 1, 0, 1]
        assert sorted(g[3] for g in r1)[2] > 0 and sorted(g[3] for g in r2)[2] > 0           # refills happened in both rounds
        for r in range(n):
            slot = r1[r][2]
            rep.begin(slot, None)
            a, _ = rep.turn(slot, P1[r], [], M1[r], one(kw, r))
            b, state = rep.turn(slot, [int(a[-1])] + tail[r], [], M2[r], one(kw, r))
            print(f"conversation {r}: turn 1 {r1[r][0].tolist()} / {a.tolist()}, turn 2 {r2[r][0].tolist()} / {b.tolist()}")
            assert r1[r][0].tolist() == a.tolist() and r2[r][0].tolist() == b.tolist()
            assert np.array_equal(bits(pool.back(r)), bits(state)), f"conversation {r}"
        pool.close()
    finally:
        rep.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 4. cut, never
def test_cut_and_never_dispatched_requests_write_nothing(ctx):
    data, V, B, mode, cap = model("small"), vocab("small"), 2, 1, 7
    P, kw = prompts(V), pick("sample", R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    save = [3, 0, 6, 1, 5, 2, 4]
    pools = []
    for _ in range(2):
        pool = wrk.StatePool(ctx, rt, R)
        for k in range(R):
            pool.load(k, pattern(rt, 7 + k))
        pools.append(pool)
    before = [pools[0].back(k) for k in range(R)]
    full, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pools[0], save_state=save, **kw)
    assert rt.last_queue_saved == [True] * R
    got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, max_steps=cap, pool=pools[1], save_state=save, **kw)
    reasons = [why for _, why, *_ in got]
    print(f"cap {cap}: reasons {reasons} saved {rt.last_queue_saved}")
    assert run == cap and Q.CAP in reasons and Q.NEVER in reasons and Q.MAX_NEW in reasons
    assert rt.last_queue_saved == PR.saved(save, reasons)
    written = PR.written(save, reasons)
    for r in range(R):
        k, have = save[r], bits(pools[1].back(save[r]))
        if k in written:        # finished under the cap: the entry holds what the uncapped call saved for it
            assert got[r][0].tolist() == full[r][0].tolist()
            assert np.array_equal(have, bits(pools[0].back(k))) and not np.array_equal(have, bits(before[k])), r
        else:
            assert np.array_equal(have, bits(before[k])), f"request {r} (reason {reasons[r]}) wrote entry {k}"
    for pool in pools:
        pool.close()
    rt.close()


# ----------------------------------------------------------------------------------------------------------------- 5. all none
@pytest.mark.parametrize("v6", [False, True])
def test_a_pool_call_with_every_index_none_equals_the_plain_call(ctx, v6):
    data, V, B, mode = model("small", v6), vocab("small", v6), 2, 1
    P, kw = prompts(V), pick("sample", R)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    zero = zero_state(rt)
    first = [5, 66]

    def others():
        for b in range(B):
            rt.state_load(zero, b)
        tok, _ = rt.generate_sample(first, 8, mode=mode, seed=[3, 4])
        return rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **kw), tok
    (plain, prun), tok = others()
    pool, before, _ = filled_pool(ctx, rt, V)
    got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, **kw)
    assert rt.last_queue_saved == [False] * R and run == prun
    assert [(t.tolist(), a, b, c) for t, a, b, c in got] == [(t.tolist(), a, b, c) for t, a, b, c in plain]
    assert all(np.array_equal(bits(pool.back(k)), bits(before[k])) for k in range(ENTRIES))
    # a call that does use the pool, then the cached plain programs again
    rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, start_state=START, save_state=SAVE, **kw)
    (again, arun), tok2 = others()
    assert arun == prun and [(t.tolist(), a, b, c) for t, a, b, c in again] == [(t.tolist(), a, b, c) for t, a, b, c in plain]
    assert np.array_equal(tok, tok2)
    pool.close()
    rt.close()


# ----------------------------------------------------------------------------------------------------------------- 6. one program
def test_one_program_serves_any_pool(ctx):
    data, V, B, mode = model("small"), vocab("small"), 2, 1
    calls = [(ENTRIES, dict(requests=prompts(V), max_new=MAX_NEW, start_state=START, save_state=SAVE, **pick("sample", R))),
             (3, dict(requests=prompts(V, [2, 4, 1], salt=3), max_new=[5, 2, 8], stop=[[1, 2], [], [V - 1]], start_state=[2, 1, 1],
                      save_state=[2, None, 0], **pick("sample", 3, salt=2))),
             (9, dict(requests=prompts(V, [1, 2, 3, 1, 2, 3, 1, 2, 3], salt=5), max_new=3, start_state=[0, 1, 2, 0, 1, 2, 0, 1, 2],
                      save_state=[8, 7, 6, 5, 4, 3, None, None, None], **pick("sample", 9, salt=1)))]      # grows the tables

    def run(rt, entries, kw):
        pool, _, _ = filled_pool(ctx, rt, V, entries, salt=entries)
        out = rt.generate_queue(mode=mode, poll_steps=POLL, pool=pool, **kw)
        back = [pool.back(k) for k in range(entries)]
        pool.close()
        return out, list(rt.last_queue_saved), back

    def fresh(entries, kw):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        out = run(rt, entries, kw)
        rt.close()
        return out
    want = [fresh(n, kw) for n, kw in calls]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    got = [run(rt, n, kw) for n, kw in calls]
    rt.close()
    for ((g, grun), gsaved, gback), ((w, wrun), wsaved, wback) in zip(got, want):
        assert grun == wrun and gsaved == wsaved
        assert [(t.tolist(), a, b, c) for t, a, b, c in g] == [(t.tolist(), a, b, c) for t, a, b, c in w]
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(gback, wback))


# ----------------------------------------------------------------------------------------------------------------- 8. validation
class FakePool:
    """what generate_queue reads of a StatePool, to put tables on the C ABI that StatePool cannot hold"""

    def __init__(self, buf, entries):
        self.buf, self.entries = buf, entries


class NoBuffer:
    h = None


@pytest.mark.parametrize("v6", [False, True])
def test_bad_pool_arguments_are_rejected_before_any_launch(ctx, v6):
    data, V, B = model("small", v6), vocab("small", v6), 2
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    other = wrk.Context(0)
    rt_other = wrk.Runtime(other, wrk.GgufReader(data), num_batch=B)
    pool, before, snaps = filled_pool(ctx, rt, V, 4)
    pool_other = wrk.StatePool(other, rt_other, 4)
    one_entry = wrk.StatePool(ctx, rt, 1)
    rt.generate_greedy([3, 4], 5)                                   # a state that is not zero
    state = [rt.state_back(b) for b in range(B)]
    good = [[1, 2], [3], [4, 5, 6]]
    ok = dict(requests=good, pool=pool)
    bad_calls = [ok | dict(start_state=[4, None, None]), ok | dict(save_state=[None, None, 4]), ok | dict(start_state=2 ** 32 - 2),
                 dict(requests=good, pool=FakePool(pool.buf, 5)), dict(requests=good, pool=FakePool(pool.buf, 3)),
                 dict(requests=good, pool=FakePool(pool.buf, 0)),
                 dict(requests=good, pool=FakePool(wrk.Buffer(ctx, pool.entry_bytes + 16), 1)),
                 dict(requests=good, pool=FakePool(NoBuffer, 4), start_state=0), dict(requests=good, pool=FakePool(NoBuffer, 4), save_state=[0, 1, 2]),
                 dict(requests=good, pool=FakePool(NoBuffer, 4)),
                 dict(requests=good, pool=one_entry, init_state=one_entry.buf),
                 ok | dict(save_state=[1, 2, 1]), ok | dict(save_state=3),                          # two savers
                 ok | dict(start_state=[None, 0, None], save_state=[0, None, None]),                # reads another request's target
                 ok | dict(start_state=[1, 0, None], save_state=[0, 1, None]),
                 dict(requests=good, pool=pool_other),
                 ok | dict(requests=[]), ok | dict(max_new=[1, 0, 2]), ok | dict(init_state=wrk.Buffer(ctx, 64))]      # the plain call's
    for kw in bad_calls:
        with pytest.raises(wrk.WrkError) as e:
            rt.generate_queue(**kw)
        assert e.value.code == wrk.E_ARG, kw
    with pytest.raises(wrk.WrkError) as e:
        rt.generate_queue(good, mode=1 | (2 << 8), pool=pool, start_state=0)                       # lanes
    assert e.value.code == wrk.E_UNSUPPORTED
    for kw in (dict(start_state=0), dict(save_state=[0, 1, 2])):
        with pytest.raises(ValueError):
            rt.generate_queue(good, **kw)                                                           # tables without a pool
    with pytest.raises(ValueError):
        rt.generate_queue(good, pool=pool, start_state=[0, 1])

    # a NULL pool, through the C ABI
    fn, mdl = (wrk.hip.wrk_v6_generate_queue_pool, rt.model6) if v6 else (wrk.hip.wrk_v7_generate_queue_pool, rt.model)
    u32p = C.POINTER(C.c_uint32)
    arrays = dict(prompt_tokens=np.array([1, 2, 3, 4], np.uint32), prompt_offsets=np.array([0, 2, 3, 4], np.uint32),
                  max_new=np.array([2, 2, 2], np.uint32))
    o = wrk.QueueOptions()
    o.num_requests, o.max_steps = 3, 32
    for k, v in arrays.items():
        setattr(o, k, v.ctypes.data_as(u32p))
    res_arrays = {k: np.zeros(8, np.uint32) for k in ("lengths", "reasons", "slots", "start_steps", "out_tokens", "steps_run")}
    res = wrk.QueueResult(*[res_arrays[k].ctypes.data_as(u32p) for k, _ in wrk.QueueResult._fields_])
    assert fn(ctx.h, mdl, rt.state, B, C.byref(o), C.byref(res), None, 1, None) == wrk.E_ARG
    for b in range(B):
        assert np.array_equal(bits(rt.state_back(b)), bits(state[b])), b
    assert all(np.array_equal(bits(pool.back(k)), bits(before[k])) for k in range(4))
    # the well-formed call the bad ones are variations of; saved may be NULL and either table too
    qp = wrk.QueuePool(pool.buf.h, 4, None, None, None)
    assert fn(ctx.h, mdl, rt.state, B, C.byref(o), C.byref(res), None, 1, C.byref(qp)) == 0
    got, _ = rt.generate_queue(good, max_new=2, pool=pool, start_state=[0, 0, 3], save_state=[None, 1, 3])
    assert rt.last_queue_saved == [False, True, True]
    for p in (pool, pool_other, one_entry):
        p.close()
    rt_other.close()
    other.close()
    rt.close()
