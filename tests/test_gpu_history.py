"""Prompt intake and the history pool of the request queue (web-rwkv-gguf_amd/csrc/wrk_queue.hip) through
`Runtime.generate_queue(count_prompt=..., history=...)` and `wrk.HistoryPool`, against tests/history_ref.py and against a replay of every
request on its own, bit for bit.

The replay is the single-request path: the request alone in the slot the queue gave it, its prompt but the last token fed by one-step
calls of the same pick kind on scratch handles, then what the contract says the context sees -- `occ.load(slot)` (the reset) or the
carried row, the slot's bans, `occ.add(slot, prompt[f:], decay)` and `win.add(slot, prompt[f:])` -- then `generate_stop` from p_{n-1} on
the real handles.  Between the turns of one conversation the handles are not reset.  What `generate_stop` leaves in the handles of a
sequence that ends is what a save writes: `occ.back(slot)` (the present bit only) and `win.back(slot)`.

Shapes: tests/test_gpu_queue_pool.py's -- synth "small" (V = 1000), R = 7 requests, prompts of 1 to 5 tokens, max_new <= 12, B in
{1, 2, 4}; windows of capacity 8, so that the rings wrap."""
import functools

import numpy as np
import pytest

import dry_ref as D
import history_ref as H
import queue_pool_ref as PR
import queue_ref as Q
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

PROMPT_LENS = [3, 1, 5, 2, 4, 1, 2]
MAX_NEW = [4, 6, 12, 5, 9, 1, 7]
R = len(PROMPT_LENS)
POLL = 4
CAP = 8
MAX_STEPS = sum(PROMPT_LENS) + sum(MAX_NEW)
# what a pick kind uses: (sampler arrays, occurrence table, token window)
KINDS = {"pen": (True, True, False), "dry": (True, False, True), "dry_greedy": (False, False, True), "all": (True, True, True)}


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def model(v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS["small"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["small"], 42)


def vocab(v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)["small"].num_vocab


def prompts(V, lens=PROMPT_LENS, salt=0):
    """a few ids only, so that prompts repeat tokens and share them with one another"""
    return [[(7 + salt + 3 * ((r + 2 * i) % 4)) % V for i in range(n)] for r, n in enumerate(lens)]


def pick(kind, n, salt=0):
    """per-request parameters of the pick kind, all different"""
    sampled, pen, dry = KINDS[kind]
    kw = {}
    if sampled:
        kw |= dict(temperature=[[1.0, 0.8, 1.2, 0.9][(r + salt) % 4] for r in range(n)], top_p=[[0.9, 1.0, 0.8, 0.95][(r + salt) % 4] for r in range(n)],
                   seed=[11 + salt + r for r in range(n)])
    if pen:
        kw |= dict(presence=[0.4 + 0.05 * r for r in range(n)], frequency=[0.6 - 0.02 * r for r in range(n)],
                   decay=[1.0 if r == 3 else 0.5 if r == 1 else 0.99 + 0.001 * r for r in range(n)])
    if dry:
        kw |= dict(dry=([[0.0, 40.0, 3.0, 25.0][(r + salt) % 4] for r in range(n)], [[1.75, 1.75, 1e30, 2.0][(r + salt) % 4] for r in range(n)],
                        [[2, 1, 1, 1][(r + salt) % 4] for r in range(n)]),
                   no_repeat_ngram=[[2, 0, 0, 3][(r + salt) % 4] if kind != "dry" else 0 for r in range(n)])
    return kw


def one(kw, r):
    return {k: (tuple(x[r] for x in v) if k == "dry" else v[r]) for k, v in kw.items()}


def zero_state(rt):
    L, D_, S = rt.info.num_layer, rt.info.num_emb, rt.info.num_emb // rt.info.num_head
    return np.zeros((L, S + 2, D_), np.float32)


class Handles:
    """the occurrence table and token window a pick kind uses (None for what it does not), and how a call names them"""

    def __init__(self, ctx, kind, B, V, cap=CAP):
        _, pen, dry = KINDS[kind]
        self.occ = wrk.Occurrence(ctx, B, V) if pen else None
        self.win = wrk.TokenWindow(ctx, B, V, cap) if dry else None
        self.B, self.V, self.cap = B, V, cap if dry else 0

    def kw(self):
        return (dict(occurrence=self.occ) if self.occ else {}) | (dict(window=self.win) if self.win else {})

    def reset(self, b):
        if self.occ:
            self.occ.load(b)
        if self.win:
            self.win.load(b)

    def set(self, b, entry, bans=()):
        """slot b <- the reset or a host entry (counts, present, window), then the slot's bans"""
        self.reset(b)
        if entry is not None and self.occ:
            self.occ.load(b, entry[0], np.asarray(entry[1], np.uint32) & 1)
        if entry is not None and self.win:
            self.win.load(b, entry[2])
        if self.occ and len(bans):
            self.occ.ban(b, bans)

    def context(self, b):
        """(counts, present, window) of slot b: what a save of the slot writes"""
        c, f = self.occ.back(b) if self.occ else (np.zeros(self.V, np.float32), np.zeros(self.V, np.uint32))
        return c, f & 1, self.win.back(b).tolist() if self.win else []

    def history(self, ctx, entries):
        return wrk.HistoryPool(ctx, entries, self.V, self.cap)

    def close(self):
        for h in (self.occ, self.win):
            if h:
                h.close()


def same_entry(have, want, what, hd):
    """a history entry against a context, over the parts the handles have"""
    if hd.occ:
        assert np.array_equal(bits(have[0]), bits(want[0])), f"{what}: counts"
        assert np.array_equal(have[1], want[1]), f"{what}: present bits"
    if hd.win:
        assert list(have[2]) == list(want[2]), f"{what}: window {list(have[2])} against {list(want[2])}"


class Replayer:
    """Replays one request alone in a slot of a runtime whose every other slot holds what a fresh runtime holds."""

    def __init__(self, ctx, data, V, B, kind, mode):
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        self.hd, self.scratch = Handles(ctx, kind, B, V), Handles(ctx, kind, B, V)
        self.V, self.B, self.kind, self.mode = V, B, kind, mode
        self.zero = zero_state(self.rt)
        self.extra = {}                 # what every call of the replay also gets (a grammar)

    def begin(self, slot, snapshot=None, entry=None, bans=()):
        for b in range(self.B):
            self.rt.state_load(self.zero, b)
            self.hd.reset(b)
        if snapshot is not None:
            self.rt.state_write(snapshot, slot)
        self.hd.set(slot, entry, bans)

    def turn(self, slot, prompt, f, stop, max_new, kw):
        """feeds `prompt` and draws the reply, continuing from what the slot and the handles hold; returns (reply, the slot's frozen
        state, the slot's context)"""
        rt, B = self.rt, self.B
        first = [(3 + 17 * b) % self.V for b in range(B)]
        none = [[] for _ in range(B)]
        for t in prompt[:-1]:           # the draws of these steps are discarded: they touch scratch handles only
            first[slot] = t
            rt.generate_stop(first, 1, none, mode=self.mode, **kw, **self.scratch.kw(), **self.extra)
        if f is not None:
            if self.hd.occ:
                self.hd.occ.add(slot, prompt[f:], kw["decay"])
            if self.hd.win:
                self.hd.win.add(slot, prompt[f:])
        first[slot] = prompt[-1]
        stops = [[] for _ in range(B)]
        stops[slot] = list(stop)
        tok, lens = rt.generate_stop(first, max_new, stops, mode=self.mode, **kw, **self.hd.kw(), **self.extra)
        return tok[:lens[slot], slot].copy(), rt.state_back(slot), self.hd.context(slot)

    def close(self):
        self.hd.close()
        self.scratch.close()
        self.rt.close()


def first_new(reply, k):
    col = [int(t) for t in reply]
    for j in list(range(k, len(col))) + list(range(k - 1, -1, -1)):
        if col[j] not in col[:j]:
            return col[j]


def forced_stops(plain, V):
    """requests 2 and 4 end mid-reply where their replies allow it, 6 ends on y_0; the others by max_new"""
    spare = next(i for i in range(V - 1, -1, -1) if all(i not in set(t.tolist()) for t, *_ in plain))
    stops = [[] for _ in range(len(plain))]
    stops[2] = [spare, first_new(plain[2][0], 3)]
    stops[4] = [first_new(plain[4][0], 2)]
    stops[6] = [int(plain[6][0][0])]
    return stops


def random_entry(V, cap, seed, n=None):
    """a finite pattern in an entry's shape: counts, present bits and a window of n tokens (default: full)"""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(V) * 3).astype(np.float32), rng.integers(0, 2, V).astype(np.uint32),
            rng.integers(0, V, cap if n is None else n).tolist())


def load_entry(hist, k, e, hd):
    hist.load(k, e[0] if hd.occ else None, e[1] if hd.occ else None, e[2] if hd.win else None)


def check_call(got, run, rep, P, f, stops, max_new, kw, B, max_steps, start=None, save=None, pool=None, hist=None, before=None, snaps=None,
               bans=None):
    """replies and schedule against the replays and queue_ref; with a pool: the state and history entries against the replays and
    history_ref's rule of which entries are written"""
    n = len(P)
    start, save = start or [None] * n, save or [None] * n
    replays = []
    for r in range(n):
        slot = got[r][2]
        rep.begin(slot, None if start[r] is None else snaps[start[r]], None if start[r] is None or hist is None else before[start[r]],
                  () if bans is None else bans[slot])
        replays.append(rep.turn(slot, P[r], None if f is None else f[r], stops[r], max_new[r], one(kw, r)))
    replies = [t for t, *_ in replays]
    want, needed = Q.run(P, replies, stops, max_new, B, max_steps)
    for r in range(n):
        t, why, slot, step = got[r]
        print(f"request {r}: slot {slot} start {step} reason {why} reply {t.tolist()} replay {replies[r].tolist()}")
        if why in (Q.STOP, Q.MAX_NEW):
            assert t.tolist() == replies[r].tolist(), f"request {r}"
        else:
            assert t.tolist() == replies[r].tolist()[:len(t)], f"request {r}"
        assert (why, slot, step) == want[r][1:], f"request {r}: {(why, slot, step)} against the schedule {want[r][1:]}"
    assert run == Q.steps_run(needed, POLL, max_steps)
    if pool is None:
        return replays
    reasons = [why for _, why, *_ in got]
    written = PR.written(save, reasons)
    for k in range(pool.entries):
        have = hist.back(k) if hist is not None else None
        if k in written:
            assert np.array_equal(bits(pool.back(k)), bits(replays[written[k]][1])), f"state entry {k}"
            if hist is not None:
                same_entry(have, replays[written[k]][2], f"history entry {k} of request {written[k]}", rep.hd)
                assert not have[1].astype(np.uint32).max() > 1, "a banned bit in an entry"
        elif hist is not None:
            same_entry(have, before[k], f"history entry {k}, named by no finished request", rep.hd)
    if hist is not None:        # and the restatement of the contract, given the replies: the same entries, the same bits
        V = rep.V
        flags = [np.zeros(V, np.uint32) for _ in range(B)]
        for b in range(B if bans is not None else 0):
            flags[b][bans[b]] = H.BANNED
        _, after, wrote = H.run(P, replies, stops, max_new, B, start, save, before, flags, f, np.ones(V, np.float32),
                                kw.get("decay", [1.0] * n), rep.hd.cap, max_steps)
        assert wrote == written
        for k in range(pool.entries):
            same_entry(hist.back(k), after[k], f"history entry {k} against history_ref", rep.hd)
    return replays


# ----------------------------------------------------------------------------------------------------------------- 1. prompt intake
def intake_identity(ctx, kind, mode, v6, B, pooled):
    data, V = model(v6), vocab(v6)
    P, kw = prompts(V), pick(kind, R)
    f = [0, 0, 2, 1, 0, 1, 5]                       # everything, a tail, nothing (f >= n)
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, kind, B, V)
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        pool = hist = before = snaps = None
        pk = {}
        if pooled:                                  # cold starts, every request saves: the contexts themselves are compared
            pool, hist = wrk.StatePool(ctx, rt, R), hd.history(ctx, R)
            before = [random_entry(V, hd.cap, 50 + k) for k in range(R)]
            for k in range(R):
                load_entry(hist, k, before[k], hd)
            before = [hist.back(k) for k in range(R)]
            pk = dict(pool=pool, history=hist, save_state=list(range(R)))
        plain, _ = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, count_prompt=f, **kw, **hd.kw())
        stops = forced_stops(plain, V)
        got, run = rt.generate_queue(P, stop=stops, max_new=MAX_NEW, mode=mode, poll_steps=POLL, count_prompt=f, **kw, **hd.kw(), **pk)
        check_call(got, run, rep, P, f, stops, MAX_NEW, kw, B, MAX_STEPS, save=pk.get("save_state"), pool=pool, hist=hist, before=before)
        reasons = [why for _, why, *_ in got]
        assert reasons[6] == Q.STOP and set(reasons) == {Q.STOP, Q.MAX_NEW}
        for h in (pool, hist):
            if h:
                h.close()
    finally:
        rep.close()
        hd.close()
        rt.close()


CONFIGS = [(kind, 1, False, B, B != 2) for kind in KINDS for B in (1, 2, 4)] + \
          [("all", 0, False, 2, True), ("all", 1, True, 1, True), ("all", 1, True, 2, False), ("all", 1, True, 4, True), ("pen", 1, True, 2, True),
           ("dry_greedy", 1, True, 2, True)]


@pytest.mark.parametrize("kind,mode,v6,B,pooled", CONFIGS)
def test_prompt_intake_equals_the_replay(ctx, kind, mode, v6, B, pooled):
    intake_identity(ctx, kind, mode, v6, B, pooled)


@pytest.mark.parametrize("kind,pooled", [("all", True), ("pen", False)])
def test_prompt_intake_equals_the_replay_eager(ctx, monkeypatch, kind, pooled):
    monkeypatch.setenv("WRK_NO_GRAPH", "1")
    intake_identity(ctx, kind, 1, False, 2, pooled)


def test_prompt_intake_equals_the_replay_engine_off(ctx, monkeypatch):
    monkeypatch.setenv("WRK_ENGINE", "0")
    intake_identity(ctx, "all", 1, False, 1, True)


# ----------------------------------------------------------------------------------------------------------------- 2. it changes something
def repeats_a_prompt_bigram(prompt, reply):
    """whether prompt ++ reply forms, with a reply token as its second id, a bigram that the prompt already holds"""
    have = {(a, b) for a, b in zip(prompt, prompt[1:])}
    seq = list(prompt) + [int(t) for t in reply]
    return any((seq[i - 1], seq[i]) in have for i in range(len(prompt), len(seq)))


@pytest.mark.parametrize("v6", [False, True])
def test_the_prompt_in_the_window_changes_a_greedy_reply(ctx, v6):
    """Greedy with no_repeat_ngram = 2, restricted to five tokens by a grammar so that replies meet their prompts (the plain loop of
    tests/test_gpu_dry.py).  Today's reply to a prompt a t a that goes on with t repeats the prompt's bigram (a, t); with the prompt in
    the window the ban sees it.  Prompt and reply are eight tokens: the ban empties no row (that takes a token with five followers)."""
    data, V, B, mode, M = model(v6), vocab(v6), 2, 1, CAP - 3        # prompt and reply fit the window: the ban forgets nothing
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, "dry_greedy", B, V)
    rep = Replayer(ctx, data, V, B, "dry_greedy", mode)
    try:
        allowed = [11, 200, 333, 77, 640]
        cls = np.zeros(V, np.uint16)
        cls[allowed] = 1
        g = wrk.Grammar(ctx, V, cls, [[wrk.GRAMMAR_REJECT, 0]])
        rep.extra = dict(grammar=g)
        call = dict(max_new=M, mode=mode, poll_steps=POLL, no_repeat_ngram=2, grammar=g, **hd.kw())
        cands = [[a, t, a] for a in allowed for t in allowed if a != t]
        today, _ = rt.generate_queue(cands, **call)
        hits = [i for i, (t, *_) in enumerate(today) if repeats_a_prompt_bigram(cands[i], t)]
        print(f"{len(hits)} of {len(cands)} candidate prompts are repeated by today's reply")
        assert hits, "no reply repeats a bigram of its prompt: the case shows nothing"
        P = [cands[i] for i in hits[:4]]
        n = len(P)
        kw = dict(no_repeat_ngram=[2] * n)
        old, _ = rt.generate_queue(P, **call)
        again, _ = rt.generate_queue(P, count_prompt=None, **call)
        got, run = rt.generate_queue(P, count_prompt=True, **call)
        for r in range(n):
            assert again[r][0].tolist() == old[r][0].tolist() and repeats_a_prompt_bigram(P[r], old[r][0]), "count_prompt=None is today's call"
            assert not repeats_a_prompt_bigram(P[r], got[r][0]) and not D.has_repeated_ngram(P[r] + got[r][0].tolist(), 3)
            assert got[r][0].tolist() != old[r][0].tolist()
        check_call(got, run, rep, P, [0] * n, [[]] * n, [M] * n, kw, B, 3 * n + M * n)
        g.close()
    finally:
        rep.close()
        hd.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 3. sessions
@pytest.mark.parametrize("kind,v6", [("all", False), ("all", True), ("pen", False), ("dry_greedy", False)])
def test_sessions_carry_their_history_across_calls(ctx, kind, v6):
    """Two turns of three conversations on two slots, each in place on its own entry of both pools.  The lengths keep every conversation
    in the same slot in both turns, so the reference -- handles and state never touched between the turns -- runs it there."""
    data, V, B, mode, n = model(v6), vocab(v6), 2, 1, 3
    kw = pick(kind, n)
    P1, M1 = prompts(V, [2, 4, 3]), [3, 6, 4]
    tail, M2 = prompts(V, [2, 4, 1], salt=3), [2, 7, 8]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, kind, B, V)
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        pool, hist = wrk.StatePool(ctx, rt, n), hd.history(ctx, n)
        own = list(range(n))
        call = dict(mode=mode, poll_steps=POLL, pool=pool, history=hist, start_state=own, save_state=own, **kw, **hd.kw())
        r1, _ = rt.generate_queue(P1, max_new=M1, count_prompt=True, **call)
        assert rt.last_queue_saved == [True] * n
        e1, s1 = [hist.back(k) for k in own], [pool.back(k) for k in own]
        P2 = [[int(r1[r][0][-1])] + tail[r] for r in range(n)]      # the last reply token was drawn, not fed: it opens the next turn
        r2, _ = rt.generate_queue(P2, max_new=M2, count_prompt=1, **call)
        assert rt.last_queue_saved == [True] * n
        e2, s2 = [hist.back(k) for k in own], [pool.back(k) for k in own]
        assert [g[2] for g in r1] == [g[2] for g in r2] == [0, 1, 0]
        for r in range(n):
            slot = r1[r][2]
            rep.begin(slot)
            a, sa, ca = rep.turn(slot, P1[r], 0, [], M1[r], one(kw, r))
            b, sb, cb = rep.turn(slot, [int(a[-1])] + tail[r], 1, [], M2[r], one(kw, r))
            print(f"conversation {r}: turn 1 {r1[r][0].tolist()} / {a.tolist()}, turn 2 {r2[r][0].tolist()} / {b.tolist()}, window {cb[2]}")
            assert r1[r][0].tolist() == a.tolist() and r2[r][0].tolist() == b.tolist()
            same_entry(e1[r], ca, f"conversation {r} after turn 1", hd)
            same_entry(e2[r], cb, f"conversation {r} after turn 2", hd)
            assert np.array_equal(bits(s1[r]), bits(sa)) and np.array_equal(bits(s2[r]), bits(sb)), f"conversation {r}: state"
            if hd.win:      # the whole conversation, each token once: the last reply token of turn 1 is not taken in twice
                assert cb[2] == (P1[r] + a.tolist() + tail[r] + b.tolist())[-CAP:]
        pool.close()
        hist.close()
    finally:
        rep.close()
        hd.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 4. / 5. one call, mixed
ENTRIES = 7
START = [None, 0, 0, 1, 2, None, None]      # 1 and 2 read entry 0, which nobody saves; 3 and 4 are in place; 6 starts cold and saves
SAVE = [None, None, 4, 1, 2, 6, 3]


def mixed_call(ctx, kind, B, mode=1, v6=False, max_steps=None):
    data, V = model(v6), vocab(v6)
    P, kw = prompts(V), pick(kind, R)
    f = [0, 1, 1, 1, 1, 0, 0]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, kind, B, V)
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        pool, hist = wrk.StatePool(ctx, rt, ENTRIES), hd.history(ctx, ENTRIES)
        zero = zero_state(rt)
        for k in range(ENTRIES):
            if k < 3:       # a conversation so far: its state, and a context that has counted it
                prefix = [(3 + 5 * i + 11 * k) % V for i in range(4 + 2 * k)]
                rt.state_load(zero, 0)
                rt.infer(wrk.RnnInput([prefix] * B, 32), mode=1)
                pool.put(k, rt.state_read(0))
                hd.set(0, None)
                if hd.occ:
                    hd.occ.add(0, prefix, 0.9)
                if hd.win:
                    hd.win.add(0, prefix)
                hist.put(k, hd.occ, 0, hd.win)
            else:           # random counts and ring contents, a partly filled ring among them
                pool.load(k, np.random.default_rng(k).standard_normal(zero.shape).astype(np.float32))
                load_entry(hist, k, random_entry(V, hd.cap, 70 + k, None if k != 5 else hd.cap // 2), hd)
        before, snaps = [hist.back(k) for k in range(ENTRIES)], [pool.get(k) for k in range(ENTRIES)]
        states = [pool.back(k) for k in range(ENTRIES)]
        steps = MAX_STEPS if max_steps is None else max_steps
        got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, max_steps=steps, count_prompt=f, pool=pool, history=hist,
                                     start_state=START, save_state=SAVE, **kw, **hd.kw())
        reasons = [why for _, why, *_ in got]
        print(f"B = {B} max_steps {steps}: reasons {reasons} saved {rt.last_queue_saved}")
        assert rt.last_queue_saved == PR.saved(SAVE, reasons)
        check_call(got, run, rep, P, f, [[]] * R, MAX_NEW, kw, B, steps, START, SAVE, pool, hist, before, snaps)
        for k in range(ENTRIES):
            if k not in PR.written(SAVE, reasons):
                assert np.array_equal(bits(pool.back(k)), bits(states[k])), f"state entry {k} changed"
        pool.close()
        hist.close()
        return got, reasons
    finally:
        rep.close()
        hd.close()
        rt.close()


@pytest.mark.parametrize("kind,B,v6", [("all", 2, False), ("all", 4, False), ("pen", 2, False), ("dry", 2, True)])
def test_one_call_mixed(ctx, kind, B, v6):
    _, reasons = mixed_call(ctx, kind, B, v6=v6)
    assert set(reasons) == {Q.MAX_NEW}


def test_cut_and_never_dispatched_requests_keep_their_entries(ctx):
    _, reasons = mixed_call(ctx, "all", 2, max_steps=13)
    assert Q.CAP in reasons and Q.NEVER in reasons and Q.MAX_NEW in reasons
    assert any(SAVE[r] is not None for r, why in enumerate(reasons) if why == Q.CAP)
    assert any(SAVE[r] is not None for r, why in enumerate(reasons) if why == Q.NEVER)


@pytest.mark.parametrize("kind,v6", [("all", False), ("pen", True)])
def test_one_slot_saves_before_it_restores(ctx, kind, v6):
    """B = 1: every turnover is the same slot ending and restarting in one step"""
    got, reasons = mixed_call(ctx, kind, 1, v6=v6)
    assert [g[2] for g in got] == [0] * R and set(reasons) == {Q.MAX_NEW}


# ----------------------------------------------------------------------------------------------------------------- 6. bans
def test_bans_stay_with_the_slot_and_out_of_the_entries(ctx):
    data, V, B, mode, kind = model(), vocab(), 2, 1, "all"
    P, kw = prompts(V), pick(kind, R)
    bans = [[P[0][0], 501, 640], [P[1][0], 502]]          # a prompt token among them: intake makes it present AND banned in the slot
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, kind, B, V)
    rep = Replayer(ctx, data, V, B, kind, mode)
    try:
        pool, hist = wrk.StatePool(ctx, rt, ENTRIES), hd.history(ctx, ENTRIES)
        for k in range(ENTRIES):
            load_entry(hist, k, random_entry(V, hd.cap, 90 + k), hd)
        before, snaps = [hist.back(k) for k in range(ENTRIES)], [pool.get(k) for k in range(ENTRIES)]
        for b in range(B):
            hd.set(b, random_entry(V, hd.cap, 7 + b), bans[b])
        got, run = rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, count_prompt=True, pool=pool, history=hist, start_state=START,
                                     save_state=SAVE, **kw, **hd.kw())
        for b in range(B):
            assert np.flatnonzero(hd.occ.back(b)[1] & 2).tolist() == sorted(bans[b]), f"slot {b}: the bans after restores and resets"
        check_call(got, run, rep, P, [0] * R, [[]] * R, MAX_NEW, kw, B, MAX_STEPS, START, SAVE, pool, hist, before, snaps, bans=bans)
        for b in range(B):
            assert not any(t in bans[b] for r in range(R) if got[r][2] == b for t in got[r][0].tolist()), "a banned token was drawn"
        for k in range(ENTRIES):
            assert int(hist.back(k)[1].max()) <= 1, f"entry {k} holds a banned bit"
        pool.close()
        hist.close()
    finally:
        rep.close()
        hd.close()
        rt.close()


# ----------------------------------------------------------------------------------------------------------------- 7. row level
@pytest.mark.parametrize("V", [1000, 1001, 1024, 1025, 4099])
@pytest.mark.parametrize("cap", [1, 4, 4096])
def test_put_get_load_back(ctx, V, cap):
    B, P = 3, 4
    occ, win, hist = wrk.Occurrence(ctx, B, V), wrk.TokenWindow(ctx, B, V, cap), wrk.HistoryPool(ctx, P, V, cap)
    rng = np.random.default_rng(V + cap)
    try:
        for k in range(P):
            c, f, w = hist.back(k)
            assert not c.any() and not f.any() and w.size == 0, "entries start empty"
        # load / back, a full and a partly filled window
        ents = [random_entry(V, cap, 3 * V + k, n) for k, n in enumerate([cap, cap // 2, 0, cap])]
        for k in range(P):
            hist.load(k, *ents[k])
        for k in range(P):
            c, f, w = hist.back(k)
            assert np.array_equal(bits(c), bits(ents[k][0])) and np.array_equal(f, ents[k][1]) and w.tolist() == ents[k][2], k
        # get keeps the slot's banned bits and nothing else of the slot
        banned = rng.choice(V, 5, replace=False).tolist()
        c0, f0 = (rng.standard_normal(V)).astype(np.float32), rng.integers(0, 2, V).astype(np.uint32)
        occ.load(1, c0, f0)
        occ.ban(1, banned)
        win.load(1, rng.integers(0, V, min(cap, 3)).tolist())
        hist.get(0, occ, 1, win)
        c, f = occ.back(1)
        want = ents[0][1].copy()
        want[banned] |= 2
        assert np.array_equal(bits(c), bits(ents[0][0])) and np.array_equal(f, want) and win.back(1).tolist() == ents[0][2]
        # a wrapped ring: pushes past the capacity, then put; the entry has the slot's order, the present bit only
        extra = rng.integers(0, V, cap // 2 + 1).tolist()
        win.add(1, extra)
        occ.add(1, extra[-3:], 0.5)
        hist.put(2, occ, 1, win)
        c, f = occ.back(1)
        hc, hf, hw = hist.back(2)
        assert np.array_equal(bits(hc), bits(c)) and np.array_equal(hf, f & 1) and hw.tolist() == win.back(1).tolist() == (ents[0][2] + extra)[-cap:]
        assert int(hf.max()) <= 1 and (f[banned] & 2).all()
        # put then get into another slot: equal backs; the other entries and slots keep their bits
        hist.get(2, occ, 2, win)
        c2, f2 = occ.back(2)
        assert np.array_equal(bits(c2), bits(c)) and np.array_equal(f2, f & 1) and win.back(2).tolist() == win.back(1).tolist()
        for k in (0, 1, 3):
            hc, hf, hw = hist.back(k)
            assert np.array_equal(bits(hc), bits(ents[k][0])) and np.array_equal(hf, ents[k][1]) and hw.tolist() == ents[k][2], k
        assert not occ.back(0)[0].any() and not occ.back(0)[1].any() and win.back(0).size == 0
        # all None: an empty entry
        hist.load(3)
        c, f, w = hist.back(3)
        assert not c.any() and not f.any() and w.size == 0
    finally:
        for h in (occ, win, hist):
            h.close()


def test_history_pool_without_windows_and_its_argument_errors(ctx):
    V, cap = 1000, 4
    occ, win, occv = wrk.Occurrence(ctx, 2, V), wrk.TokenWindow(ctx, 2, V, cap), wrk.Occurrence(ctx, 2, V + 4)
    win8 = wrk.TokenWindow(ctx, 2, V, 8)
    rows, both = wrk.HistoryPool(ctx, 2, V), wrk.HistoryPool(ctx, 2, V, cap)
    occ.add(0, [5, 5, 9], 0.5)
    rows.put(1, occ, 0)
    c, f, w = rows.back(1)
    assert c[5] == 0.75 and c[9] == 1.0 and f.sum() == 2 and w.size == 0      # (1 * 0.5 + 1) * 0.5, then the 9
    rows.get(1, occ, 1)
    assert np.array_equal(occ.back(1)[0], c)
    both.put(0, None, 0, win)                       # a window alone
    want = [both.back(k) for k in range(2)], [rows.back(k) for k in range(2)]
    bad = [lambda: rows.put(2, occ, 0), lambda: rows.put(0, occ, 2), lambda: rows.put(0), lambda: rows.put(0, occ, 0, win),
           lambda: both.put(0, occ, 0), lambda: both.get(0, occ, 0, win8), lambda: rows.get(0, occv, 0), lambda: both.load(0, tokens=[1] * 5),
           lambda: both.load(0, tokens=[V]), lambda: rows.load(0, tokens=[1]), lambda: rows.load(0, np.zeros(V, np.float32), np.full(V, 2)),
           lambda: rows.load(0, np.full(V, np.inf, np.float32), np.zeros(V)), lambda: rows.back(2)]
    for call in bad:
        with pytest.raises(wrk.WrkError) as e:
            call()
        assert e.value.code == wrk.E_ARG
    for u32 in (0, wrk.MAX_TOKEN_WINDOW + 1):
        with pytest.raises(wrk.WrkError):
            wrk.HistoryPool(ctx, *((0, V, 0) if u32 == 0 else (2, V, u32)))
    have = [both.back(k) for k in range(2)], [rows.back(k) for k in range(2)]
    for a, b in zip(want[0] + want[1], have[0] + have[1]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for h in (occ, win, occv, win8, rows, both):
        h.close()


# ----------------------------------------------------------------------------------------------------------------- 8. unchanged calls
@pytest.mark.parametrize("v6", [False, True])
def test_existing_calls_are_unchanged_by_a_history_call(ctx, v6):
    data, V, B, steps, mode = model(v6), vocab(v6), 3, 10, 1
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    hd = Handles(ctx, "all", B, V)
    occ, win = hd.occ, hd.win
    zero = zero_state(rt)
    first = [5, 66, 127 % V]
    skw = dict(temperature=[1.0, 0.8, 1.2], top_p=[0.9, 1.0, 0.8], seed=[11, 12, 13])
    pkw = dict(presence=0.3, frequency=0.2, decay=0.996)
    P, qkw = prompts(V), pick("all", R)
    pool = wrk.StatePool(ctx, rt, ENTRIES)

    def loops():
        out = []
        for call in (lambda: rt.generate_greedy(first, steps, mode=mode)[0],
                     lambda: rt.generate_sample(first, steps, mode=mode, **skw)[0],
                     lambda: rt.generate_penalized(first, steps, occ, mode=mode, **skw, **pkw)[0],
                     lambda: rt.generate_stop(first, steps, [[], [9], []], mode=mode, occurrence=occ, window=win, no_repeat_ngram=2, **skw, **pkw)[0],
                     lambda: rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, **qkw, **hd.kw()),
                     lambda: rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, start_state=START, save_state=SAVE,
                                               **qkw, **hd.kw())):
            for b in range(B):
                rt.state_load(zero, b)
                hd.reset(b)
            for k in range(ENTRIES):
                pool.load(k, np.full(zero.shape, 0.01 * k, np.float32))
            res = call()
            toks = [res.copy()] if isinstance(res, np.ndarray) else [t for t, *_ in res[0]] + [np.array([g[1:] for g in res[0]]), np.array(res[1])]
            out.append(toks + [rt.state_back(b) for b in range(B)] + [pool.back(k) for k in range(ENTRIES)])
        return out
    before = loops()
    hist = hd.history(ctx, ENTRIES)
    rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, count_prompt=True, **qkw, **hd.kw())
    rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, count_prompt=1, pool=pool, history=hist, start_state=START, save_state=SAVE,
                      **qkw, **hd.kw())
    rt.generate_queue(P, max_new=MAX_NEW, mode=mode, poll_steps=POLL, pool=pool, history=hist, start_state=START, save_state=SAVE, **qkw, **hd.kw())
    after = loops()
    for h in (hist, pool, hd, rt):
        h.close()
    for a, b in zip(before, after):
        assert len(a) == len(b) and all(np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)
                                        for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------- 9. argument errors
class FakeHistory:
    h = None


@pytest.mark.parametrize("v6", [False, True])
def test_bad_history_arguments_are_rejected_before_any_launch(ctx, v6):
    data, V, B, n = model(v6), vocab(v6), 2, 4
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    other = wrk.Context(0)
    occ, win, win4 = wrk.Occurrence(ctx, B, V), wrk.TokenWindow(ctx, B, V, CAP), wrk.TokenWindow(ctx, B, V, 4)
    pool = wrk.StatePool(ctx, rt, n)
    both, rows, three = wrk.HistoryPool(ctx, n, V, CAP), wrk.HistoryPool(ctx, n, V), wrk.HistoryPool(ctx, 3, V, CAP)
    vocab4, foreign = wrk.HistoryPool(ctx, n, V + 4, CAP), wrk.HistoryPool(other, n, V, CAP)
    hists = [both, rows, three, vocab4]
    for h in hists:
        for k in range(h.entries):
            h.load(k, *random_entry(h.num_vocab, h.capacity, 11 + k))
    rt.generate_greedy([3, 4], 5)                                   # a state that is not zero
    for b in range(B):
        occ.load(b, *random_entry(V, 0, 30 + b)[:2])
        win.load(b, [1 + b, 2, 3])
        win4.load(b, [4, 5 + b])

    def everything():
        return ([rt.state_back(b) for b in range(B)] + [pool.back(k) for k in range(n)] + [x for b in range(B) for x in occ.back(b)]
                + [win.back(b) for b in range(B)] + [win4.back(b) for b in range(B)] + [x for h in hists for k in range(h.entries) for x in h.back(k)])
    before = everything()
    good = [[1, 2], [3], [4, 5, 6]]
    samp = dict(temperature=1.0, top_p=0.9, seed=[1, 2, 3])
    ok = dict(requests=good, pool=pool, start_state=[0, None, 1], save_state=[0, 2, None])
    bad_calls = [ok | dict(history=both),                                                            # neither a table nor a window
                 ok | dict(history=both, **samp),
                 ok | dict(history=foreign, occurrence=occ, window=win, **samp),                     # another context
                 ok | dict(history=vocab4, occurrence=occ, window=win, **samp),                      # another vocabulary
                 ok | dict(history=three, occurrence=occ, window=win, **samp),                       # another entry count
                 ok | dict(history=both, occurrence=occ, window=win4, **samp),                       # windows of another capacity
                 ok | dict(history=rows, occurrence=occ, window=win, **samp),                        # a window, a history without windows
                 ok | dict(history=both, occurrence=occ, **samp),                                    # a history with windows, no window
                 ok | dict(history=both, window=win, save_state=[0, 0, None]),                       # the pool's own rules still hold
                 dict(requests=good, count_prompt=True), dict(requests=good, count_prompt=[0, 1, 2], **samp)]       # intake into nothing
    for kw in bad_calls:
        with pytest.raises(wrk.WrkError) as e:
            rt.generate_queue(**kw)
        assert e.value.code == wrk.E_ARG, kw
    with pytest.raises(wrk.WrkError) as e:
        rt.generate_queue(good, history=both, window=win)                                            # a history without a pool
    assert e.value.code == wrk.E_ARG
    with pytest.raises(ValueError):
        rt.generate_queue(good, window=win, count_prompt=[0, 1])
    after = everything()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b)
    # the well-formed calls the bad ones are variations of
    rt.generate_queue(**(ok | dict(history=both, occurrence=occ, window=win, count_prompt=1, **samp)))
    rt.generate_queue(**(ok | dict(history=rows, occurrence=occ, **samp)))
    rt.generate_queue(**(ok | dict(history=both, window=win)))
    assert rt.last_queue_saved == [True, True, False]
    for h in hists + [foreign, occ, win, win4]:
        h.close()
    pool.close()
    rt.close()
    other.close()
