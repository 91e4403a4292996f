"""DRY and the no-repeat-n-gram ban on the device (web-rwkv-gguf_amd/csrc/wrk_dry.hip) against the restatement in
tests/dry_ref.py: the row function (`Context.dry_logits`) and the token window bit for bit, and a window in every decode loop
(`generate_greedy` / `_sample` / `_penalized` / `_stop` / `_queue`, with and without a state pool) of both runners.

The loops run on the tiny fixtures (V = 512).  A loop call must equal a host-driven replay: one-step calls that return the head output,
then `penalize_logits`, `dry_logits`, `constrain_logits` and the row sampler with the call's seed and step, the draw pushed into a second
window from the host; tokens, lengths and final windows are compared exactly.  Every case also asserts that its tokens differ from the
same call without DRY, so that none passes vacuously: the generate cases pre-load each window so that the first plain draw is the token
DRY acts on; the queue cases, whose windows start empty, restrict the replies to three tokens with a one-state grammar (the CPU oracle's
plain replies then repeat a bigram within six tokens for nine of ten request / model pairs).

A wrk_buf always starts at its allocation, so a misaligned base cannot reach the row function through the ABI; rows at misaligned
addresses are reached with a stride that is no multiple of four."""
import ctypes as C
import functools

import numpy as np
import pytest

import dry_ref as D
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
QNAN = [0x7FC01234, 0xFFC00001]             # quiet NaN payloads: a touched NaN keeps them through the subtraction on every IEEE machine
SPECIAL = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x477FE000, 0xC77FE000,
                    0x00000001, 0x807FFFFF, 0x00800000, 0x7F7FFFFF], np.uint32)
TOUCHED = np.array(QNAN + [0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0xC1200000, 0x00000001],
                   np.uint32)
# (multiplier, base, allowed_length, no_repeat_ngram): all off; the defaults with a multiplier; a penalty that clamps; the three bans; mixed
PARAMS = [(0.0, 1.75, 2, 0), (0.8, 1.75, 2, 0), (3.0, 1e30, 1, 0), (0.0, 1.75, 2, 2), (1.0, 2.0, 3, 3), (0.5, 1.0, 50, 51), (2.0, 1.5, 1, 51),
          (1.0, 1.75, 4, 0)]


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def matches(window, breakers):
    return D.match_lengths(window, breakers)


def exact_match(length):
    """A window whose one candidate matches exactly `length` tokens (before the cap): the earlier copy is preceded by another token."""
    body = list(range(100, 100 + length))
    return [1] + body + [9, 2] + body


def windows_for(cap, V, rng):
    """[(tokens pushed in order, pieces they are pushed in)]: the window is the last `cap` of them."""
    small = lambda n: rng.integers(0, min(3, V), n).tolist()
    out = [([], 1), (small(1), 1), ([2 % V, 2 % V], 1)]
    if cap > 2:
        out += [(small(cap - 1), 1), (small(cap), 2), (small(cap + cap // 2 + 3), 3)]           # the last one wraps the ring
    else:
        out += [(small(cap), 1), (small(3 * cap + 1), 2)]
    if cap == wrk.MAX_TOKEN_WINDOW:
        out += [([4 % V] * cap, 1), ([1, 2] * (cap // 2), 1), ([1, 0, 2, 1, 0, 2], 1), ([1, 2, 0, 1, 2], 1), ([0, 3, 0], 1)]
        if V > 200:
            out += [(exact_match(n), 1) for n in (49, 50, 51)]
    return out


def row_values(rng, n, stride, V, touched):
    """Random rows with special bit patterns sprinkled in; the tokens DRY may touch cycle through TOUCHED."""
    a = rng.normal(0, 3, (n, stride)).astype(np.float32)
    u = a.view(np.uint32)
    where = rng.random(a.shape) < 0.25
    u[where] = rng.choice(SPECIAL, int(where.sum()))
    for r in range(n):
        for k, t in enumerate(sorted(touched[r])):
            if t < V:
                u[r, t] = TOUCHED[(k + r) % TOUCHED.size]
    return a


@pytest.mark.parametrize("V,cap", [(5, 1), (5, 2), (64, 64), (64, 2), (4099, 64), (4099, 4096), (65536, 4096), (65536, 1)])
def test_dry_logits_matches_the_restatement(ctx, V, cap):
    rng = np.random.default_rng(1000 * cap + V)
    pushed = windows_for(cap, V, rng)
    n = len(pushed)
    win = wrk.TokenWindow(ctx, n, V, cap)
    want_w = []
    for r, (tok, pieces) in enumerate(pushed):
        if pieces == 1 and len(tok) <= cap:
            win.load(r, tok)
        else:
            for part in np.array_split(np.asarray(tok, np.uint32), pieces):
                win.add(r, part)
        want_w.append(tuple(tok[-cap:]))
        assert win.back(r).tolist() == list(want_w[r]), (r, "the window holds the last pushes, oldest first")
    par = [PARAMS[(r + cap) % len(PARAMS)] for r in range(n)]
    par[2] = PARAMS[0]                                                                  # an all-off row in every call, on a window that matches
    mult, base, allowed, nr = ([p[k] for p in par] for k in range(4))
    for breakers in ((), (0,), (2 % V, 0, V - 1)):
        touched = [set(matches(w, breakers)) for w in want_w]
        for stride in (V, V + 3, V + 8):
            a = row_values(rng, n, stride, V, touched)
            buf = ctx.buffer(a)
            assert ctx.dry_logits(buf, win, dry=(mult, base, allowed), no_repeat_ngram=nr, dry_breakers=list(breakers), num_vocab=V,
                                  row_stride=stride) is None
            got = buf.read(np.float32, a.size).reshape(n, stride)
            for r in range(n):
                want = D.dry_row(a[r, :V], want_w[r], *par[r], breakers=breakers, matched=matches(want_w[r], breakers))
                assert np.array_equal(bits(got[r, :V]), bits(want)), (breakers, stride, r, par[r])
                assert np.array_equal(bits(got[r, V:]), bits(a[r, V:])), "the padding between rows is not touched"
                if par[r] == PARAMS[0]:
                    assert np.array_equal(bits(got[r]), bits(a[r])), "an all-off row is its input"
        assert all(win.back(r).tolist() == list(want_w[r]) for r in range(n))
    # the cases reach what they are there for
    if cap == wrk.MAX_TOKEN_WINDOW:
        assert max(matches(want_w[6], ()).values()) == D.MAX_MATCH == max(matches(want_w[7], ()).values())
        assert matches(want_w[8], (0,)) == {1: 1} and matches(want_w[9], (0,)) == {} and matches(want_w[10], (0,)) == {}
    if cap == wrk.MAX_TOKEN_WINDOW and V > 200:
        assert [matches(want_w[11 + k], ()) for k in range(3)] == [{9: 49}, {9: 50}, {9: 50}]
    # first_batch: rows 0.. of the logits on slots 2.. of the window; defaults for the arrays that are None
    if n > 3:
        a = row_values(rng, n - 2, V, V, [set(matches(w, ())) for w in want_w[2:]])
        got = ctx.dry_logits(a, win, no_repeat_ngram=2, first_batch=2)
        assert all(np.array_equal(bits(got[r]), bits(D.dry_row(a[r], want_w[r + 2], no_repeat_ngram=2))) for r in range(n - 2))
        got = ctx.dry_logits(a, win, dry=(0.7, 1.75, 2), first_batch=2)
        assert all(np.array_equal(bits(got[r]), bits(D.dry_row(a[r], want_w[r + 2], 0.7, 1.75, 2))) for r in range(n - 2))
    win.close()


def test_window_and_row_function_argument_errors(ctx):
    V = 50
    win = wrk.TokenWindow(ctx, 2, V, 8)
    win.load(0, [1, 2, 3])
    x = np.zeros((2, V), np.float32)
    other_ctx = wrk.Context(0)
    foreign = wrk.TokenWindow(other_ctx, 2, V, 8)
    bad = [lambda: win.add(0, [V]), lambda: win.load(0, [0] * 9), lambda: win.load(0, [V]), lambda: win.add(2, [1]), lambda: win.back(2),
           lambda: ctx.dry_logits(x, win, dry=(-1.0, 1.75, 2)), lambda: ctx.dry_logits(x, win, dry=(np.inf, 1.75, 2)),
           lambda: ctx.dry_logits(x, win, dry=(np.nan, 1.75, 2)), lambda: ctx.dry_logits(x, win, dry=(1.0, 0.5, 2)),
           lambda: ctx.dry_logits(x, win, dry=(1.0, np.inf, 2)), lambda: ctx.dry_logits(x, win, dry=(1.0, 1.75, 0)),
           lambda: ctx.dry_logits(x, win, dry=(1.0, 1.75, 51)), lambda: ctx.dry_logits(x, win, no_repeat_ngram=1),
           lambda: ctx.dry_logits(x, win, no_repeat_ngram=[0, 52]), lambda: ctx.dry_logits(x, win, dry_breakers=[V]),
           lambda: ctx.dry_logits(x, win, dry_breakers=list(range(17))), lambda: ctx.dry_logits(x, win, first_batch=1),
           lambda: ctx.dry_logits(np.zeros((1, V + 1), np.float32), win), lambda: ctx.dry_logits(x, foreign),
           lambda: wrk.TokenWindow(ctx, 0, V, 8), lambda: wrk.TokenWindow(ctx, 2, 0, 8), lambda: wrk.TokenWindow(ctx, 2, V, 0),
           lambda: wrk.TokenWindow(ctx, 2, V, wrk.MAX_TOKEN_WINDOW + 1)]
    for k, call in enumerate(bad):
        with pytest.raises(wrk.WrkError) as e:
            call()
        assert e.value.code == wrk.E_ARG, k
    with pytest.raises(wrk.WrkError) as e:
        wrk.TokenWindow(ctx, 1, 2 ** 20 + 1, 8)
    assert e.value.code == wrk.E_UNSUPPORTED
    assert win.back(0).tolist() == [1, 2, 3] and win.back(1).tolist() == []
    ctx.dry_logits(x, win, dry=(0.0, 1.0, 50), no_repeat_ngram=51, dry_breakers=list(range(16)))      # the edges of every range
    win.load(0)
    assert win.back(0).tolist() == []
    foreign.close()
    other_ctx.close()
    win.close()


# ----------------------------------------------------------------------------- the loops
# (v6, mode, B, eager): RWKV-7's engine, fused, op-by-op and eager steps, RWKV-6 fused and op-by-op
CONFIGS = [(False, 1, 1, False), (False, 1, 3, False), (False, 0, 2, False), (False, 1, 2, True), (True, 1, 2, False), (True, 0, 2, False)]
FIRST = [7, 100, 300, 411]
STEPS = 7
CAP = 6                                     # smaller than pre-load + steps: the ring wraps inside the loop
SAMPLER = dict(temperature=[0.8, 1.0, 1.3, 0.9], top_p=[0.9, 1.0, 1.0, 0.7], seed=[61, 62, 63, 64])
PEN = dict(presence=[0.4, 1.5, -0.2, 0.3], frequency=[0.3, 0.0, 0.6, 0.2], decay=[0.996, 1.0, 0.5, 0.9])
# per sequence: a ban, DRY with the defaults' shape, DRY that clamps, both
DRY = dict(dry=([0.0, 40.0, 3.0, 25.0], [1.75, 1.75, 1e30, 2.0], [2, 2, 1, 1]), no_repeat_ngram=[2, 0, 0, 3], dry_breakers=[5])


@functools.lru_cache(maxsize=None)
def model(v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)


def vocab(v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)["tiny"].num_vocab


def fresh(ctx, v6, B):
    return wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=B)


def zero_states(rt, B):
    z = np.zeros_like(rt.state_back(0))
    for b in range(B):
        rt.state_load(z, b)


def cut(kw, B):
    return {k: (tuple(x[:B] for x in v) if k == "dry" else v if k == "dry_breakers" else v[:B]) for k, v in kw.items()}


def preload(plain_first, b):
    """A window that makes the sequence's first plain draw p the token every row of DRY acts on: ... 8 9 p 8 9, with M[p] = 2."""
    p = int(plain_first)
    a, c = (8 + b) % 500 + 6, (9 + 2 * b) % 500 + 6
    return [a, c, p, a, c]


def loop_call(rt, family, B, mode, first, steps, stop=None, occ=None, **extra):
    zero_states(rt, B)
    kw = {} if family == "greedy" else cut(SAMPLER, B)
    if family == "pen":
        for b in range(B):
            occ.load(b)
        kw |= cut(PEN, B)
    if stop is not None:
        if family == "pen":
            kw["occurrence"] = occ
        tok, lens = rt.generate_stop(first, steps, stop, mode=mode, **kw, **extra)
        return tok, lens
    if family == "greedy":
        return rt.generate_greedy(first, steps, mode=mode, **extra)[0], None
    if family == "pen":
        return rt.generate_penalized(first, steps, occ, mode=mode, **kw, **extra)[0], None
    return rt.generate_sample(first, steps, mode=mode, **kw, **extra)[0], None


class Host:
    """The host-driven loop: a runtime of its own that is stepped one token at a time, the row functions applied to the head output."""

    def __init__(self, ctx, v6, B, mode, cap):
        self.ctx, self.B, self.mode, self.V = ctx, B, mode, vocab(v6)
        self.rt = fresh(ctx, v6, B)
        self.win = wrk.TokenWindow(ctx, B, self.V, cap)
        self.off = wrk.TokenWindow(ctx, B, self.V, 1)      # the one-step calls run the loop's own kind of step, with nothing switched on
        self.occ = wrk.Occurrence(ctx, B, self.V)

    def head(self, cur):
        return self.rt.generate_greedy(cur, 1, mode=self.mode, want_logits=True, window=self.off)[2]

    def pick(self, x, rows, sampler, steps_of):
        """The draw of logits rows `rows` (sequence ids) at their sampler steps."""
        if sampler is None:
            return [int(np.argmax(x[k])) for k in range(len(rows))]
        return [int(self.ctx.sample_logits(x[k:k + 1], sampler["temperature"][b], sampler["top_p"][b], sampler["seed"][b], step=steps_of[k])[0])
                for k, b in enumerate(rows)]

    def generate(self, family, first, steps, windows, dry_kw, stop=None, grammar=None):
        B = self.B
        zero_states(self.rt, B)
        for b in range(B):
            self.win.load(b, windows[b])
            self.occ.load(b)
        sampler = None if family == "greedy" else cut(SAMPLER, B)
        pen = cut(PEN, B) if family == "pen" else None
        cur, toks, lens = list(first), [], [None] * B
        for step in range(steps):
            x = self.head(cur)
            if pen:
                x = self.ctx.penalize_logits(x, self.occ, pen["presence"], pen["frequency"])
            x = self.ctx.dry_logits(x, self.win, **dry_kw)
            if grammar is not None:
                x = self.ctx.constrain_logits(x, grammar, 0)
            y = self.pick(x, list(range(B)), sampler, [step] * B)
            for b in range(B):
                if lens[b] is not None:
                    continue                            # a finished sequence: its draws no longer count
                self.win.add(b, [y[b]])
                if pen:
                    self.occ.add(b, [y[b]], pen["decay"][b])
                if stop is not None and y[b] in stop[b]:
                    lens[b] = step + 1
            toks.append(y)
            cur = y
        return np.array(toks, np.uint32), [steps if n is None else n for n in lens], [self.win.back(b).tolist() for b in range(B)]

    def request(self, slot, prompt, max_new, stop, sampler, dry_kw, grammar):
        """One queue request alone in its slot: the prompt at decode rate, then its reply on a window that starts empty."""
        B = self.B
        zero_states(self.rt, B)
        self.win.load(slot)
        cur = [(3 + 17 * b) % self.V for b in range(B)]
        for t in prompt[:-1]:
            cur[slot] = int(t)
            self.head(cur)
        cur[slot] = int(prompt[-1])
        reply = []
        for j in range(max_new):
            x = self.head(cur)[slot:slot + 1]
            x = self.ctx.dry_logits(x, self.win, first_batch=slot, **dry_kw)
            if grammar is not None:
                x = self.ctx.constrain_logits(x, grammar, 0)
            y = int(np.argmax(x[0])) if sampler is None else int(self.ctx.sample_logits(x, *sampler, step=j)[0])
            self.win.add(slot, [y])
            reply.append(y)
            cur[slot] = y
            if y in stop:
                break
        return reply

    def close(self):
        for h in (self.win, self.off, self.occ):
            h.close()
        self.rt.close()


@pytest.mark.parametrize("v6,mode,B,eager", CONFIGS)
def test_generate_loops_equal_the_host_driven_replay(ctx, monkeypatch, v6, mode, B, eager):
    if eager:
        monkeypatch.setenv("WRK_NO_GRAPH", "1")
    V = vocab(v6)
    rt, host = fresh(ctx, v6, B), Host(ctx, v6, B, mode, CAP)
    win, occ = wrk.TokenWindow(ctx, B, V, CAP), wrk.Occurrence(ctx, B, V)
    first, dry_kw = FIRST[:B], cut(DRY, B)
    for family in ("greedy", "sample", "pen"):
        plain, _ = loop_call(rt, family, B, mode, first, STEPS, occ=occ)
        windows = [preload(plain[0, b], b) for b in range(B)]
        for b in range(B):
            win.load(b, windows[b])
        got, _ = loop_call(rt, family, B, mode, first, STEPS, occ=occ, window=win, **dry_kw)
        assert all(got[0, b] != plain[0, b] for b in range(B)), (family, "DRY changed no first draw: the case shows nothing")
        want, _, want_w = host.generate(family, first, STEPS, windows, dry_kw)
        assert np.array_equal(got, want), family
        assert [win.back(b).tolist() for b in range(B)] == want_w, family
        assert all(want_w[b] == (windows[b] + got[:, b].tolist())[-CAP:] for b in range(B)), "every draw was pushed, x_0 was not"
        # with stop sets: sequence 0 ends on its fourth DRY token, its window freezes there; pushes equal lengths
        stops = [[int(got[3, 0])]] + [[] for _ in range(B - 1)]
        for b in range(B):
            win.load(b, windows[b])
        cut_tok, lens = loop_call(rt, family, B, mode, first, STEPS, stop=stops, occ=occ, window=win, poll_steps=2, **dry_kw)
        want, want_len, want_w = host.generate(family, first, STEPS, windows, dry_kw, stop=stops)
        assert lens.tolist() == want_len and lens[0] <= 4, family
        for b in range(B):
            assert cut_tok[:lens[b], b].tolist() == want[:lens[b], b].tolist() == got[:lens[b], b].tolist(), (family, b)
            assert win.back(b).tolist() == want_w[b] == (windows[b] + got[:lens[b], b].tolist())[-CAP:], (family, b, "pushes equal out_lengths")
    # a window with every parameter array None records the draws and changes none
    plain, _ = loop_call(rt, "greedy", B, mode, first, STEPS)
    for b in range(B):
        win.load(b)
    got, _ = loop_call(rt, "greedy", B, mode, first, STEPS, window=win)
    assert np.array_equal(got, plain) and all(win.back(b).tolist() == plain[-CAP:, b].tolist() for b in range(B))
    for h in (win, occ, host, rt):
        h.close()


ALLOWED = [11, 200, 333]
PROMPT_LENS = [3, 1, 2, 2, 1]
MAX_NEW = [6, 5, 6, 4, 6]


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("v6,mode,B,eager", CONFIGS)
def test_queue_equals_the_host_driven_replay(ctx, monkeypatch, v6, mode, B, eager, pool):
    if eager:
        monkeypatch.setenv("WRK_NO_GRAPH", "1")
    V, R = vocab(v6), len(PROMPT_LENS)
    cls = np.zeros(V, np.uint16)
    cls[ALLOWED] = 1
    g = wrk.Grammar(ctx, V, cls, [[wrk.GRAMMAR_REJECT, 0]])
    prompts = [[(7 + 13 * r + 29 * i) % V for i in range(n)] for r, n in enumerate(PROMPT_LENS)]
    # per request: a ban, DRY, DRY that clamps, all off, both
    dry_kw = dict(dry=([0.0, 40.0, 3.0, 0.0, 25.0], [1.75, 1.75, 1e30, 1.75, 2.0], [2, 1, 1, 2, 1]), no_repeat_ngram=[2, 0, 0, 0, 3])
    rt, host = fresh(ctx, v6, B), Host(ctx, v6, B, mode, CAP)
    win = wrk.TokenWindow(ctx, B, V, CAP)
    sp = wrk.StatePool(ctx, rt, R) if pool else None
    pk = dict(pool=sp, save_state=list(range(R))) if pool else {}
    differs = 0
    for family in ("greedy", "sample"):
        kw = {} if family == "greedy" else {k: np.resize(v, R) for k, v in SAMPLER.items()}
        plain, _ = rt.generate_queue(prompts, max_new=MAX_NEW, mode=mode, poll_steps=4, grammar=g, **kw, **pk)
        for b in range(B):
            win.load(b, [ALLOWED[0], ALLOWED[1], ALLOWED[0]])      # what a slot held does not reach its request: the window starts empty
        got, _ = rt.generate_queue(prompts, max_new=MAX_NEW, mode=mode, poll_steps=4, grammar=g, window=win, **dry_kw, **kw, **pk)
        assert len({x[2] for x in got}) == B and [x[1] for x in got] == [2] * R
        for r in range(R):
            one = dict(dry=tuple(v[r] for v in dry_kw["dry"]), no_repeat_ngram=dry_kw["no_repeat_ngram"][r])
            sampler = None if family == "greedy" else [kw[k][r] for k in ("temperature", "top_p", "seed")]
            want = host.request(got[r][2], prompts[r], MAX_NEW[r], [], sampler, one, g)
            assert got[r][0].tolist() == want, (family, r, "whatever slot and step served the request")
            differs += got[r][0].tolist() != plain[r][0].tolist()
            if dry_kw["no_repeat_ngram"][r] == 2:
                assert not D.has_repeated_ngram(want, 2)
        assert got[3][0].tolist() == plain[3][0].tolist(), "the all-off request is the plain one"
    assert differs >= 2, "DRY changed no reply: the case shows nothing"
    for h in (win, host, g, rt) + ((sp,) if sp else ()):
        h.close()


@pytest.mark.parametrize("v6,mode,B", [(False, 1, 1), (False, 0, 2), (True, 1, 2)])
def test_greedy_with_the_bigram_ban_repeats_no_bigram(ctx, v6, mode, B):
    """Greedy with no_repeat_ngram = 2 and no breakers, restricted to four tokens by a grammar so that the plain loop repeats.  Seven
    steps: the ban empties a row only once the last token has had four different followers, which takes eight tokens."""
    V = vocab(v6)
    allowed = ALLOWED + [77]
    cls = np.zeros(V, np.uint16)
    cls[allowed] = 1
    g = wrk.Grammar(ctx, V, cls, [[wrk.GRAMMAR_REJECT, 0]])
    rt = fresh(ctx, v6, B)
    win = wrk.TokenWindow(ctx, B, V, 64)
    plain, _ = rt.generate_greedy(FIRST[:B], 7, mode=mode, grammar=g)
    zero_states(rt, B)
    got, _ = rt.generate_greedy(FIRST[:B], 7, mode=mode, grammar=g, window=win, no_repeat_ngram=2)
    assert any(D.has_repeated_ngram(plain[:, b], 2) for b in range(B)), "the plain loop repeats no bigram: the case shows nothing"
    for b in range(B):
        assert not D.has_repeated_ngram(got[:, b], 2) and set(got[:, b].tolist()) <= set(allowed), b
        assert win.back(b).tolist() == got[:, b].tolist()
    for h in (win, g, rt):
        h.close()


def test_lanes_do_not_change_tokens_or_windows(ctx):
    V, B = vocab(), 4
    rt = fresh(ctx, False, B)
    win = wrk.TokenWindow(ctx, B, V, CAP)
    plain, _ = loop_call(rt, "sample", B, 1, FIRST, STEPS)
    windows = [preload(plain[0, b], b) for b in range(B)]
    out = []
    for groups in (1, 2):
        for b in range(B):
            win.load(b, windows[b])
        tok, _ = loop_call(rt, "sample", B, 1, FIRST, STEPS, window=win, groups=groups, **DRY)
        out.append((tok, [win.back(b).tolist() for b in range(B)]))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
    assert not np.array_equal(out[0][0], plain)
    win.close()
    rt.close()


def test_argument_errors_leave_state_and_window_untouched(ctx):
    V = vocab()
    rt = fresh(ctx, False, 2)
    win = wrk.TokenWindow(ctx, 2, V, 8)
    small = wrk.TokenWindow(ctx, 1, V, 8)
    other_vocab = wrk.TokenWindow(ctx, 2, V + 1, 8)
    other_ctx = wrk.Context(0)
    foreign = wrk.TokenWindow(other_ctx, 2, V, 8)
    rt.generate_greedy([1, 2], 3)
    win.load(0, [4, 5, 4])
    before = rt.state_back(0).copy()
    bad = [dict(window=small), dict(window=other_vocab), dict(window=foreign), dict(window=win, dry_breakers=[V]),
           dict(window=win, dry_breakers=list(range(17))), dict(window=win, dry=(-1.0, 1.75, 2)), dict(window=win, dry=(np.nan, 1.75, 2)),
           dict(window=win, dry=(1.0, 0.9, 2)), dict(window=win, dry=(1.0, np.inf, 2)), dict(window=win, dry=(1.0, 1.75, 0)),
           dict(window=win, dry=(1.0, 1.75, 51)), dict(window=win, no_repeat_ngram=1), dict(window=win, no_repeat_ngram=[2, 52])]
    for kw in bad:
        for call in (lambda: rt.generate_greedy([1, 2], 3, **kw), lambda: rt.generate_sample([1, 2], 3, **kw),
                     lambda: rt.generate_stop([1, 2], 3, [5], **kw), lambda: rt.generate_queue([[1, 2], [3]], max_new=2, **kw)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, kw
    with pytest.raises(ValueError):
        rt.generate_greedy([1, 2], 3, dry=(1.0, 1.75, 2))
    # parameter and breaker arrays without a window, through the ABI
    ft, arr, f32 = np.array([1, 2], np.uint32), np.array([2, 2], np.uint32), np.ones(2, np.float32)
    out, lens, run = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32), C.c_uint32()
    for field, a, ty in (("dry_multiplier", f32, wrk._f32p), ("dry_base", f32, wrk._f32p), ("dry_allowed_length", arr, wrk._u32p),
                         ("no_repeat_ngram", arr, wrk._u32p), ("dry_breakers", arr, wrk._u32p)):
        opt = wrk.GenerateOptions()
        setattr(opt, field, P_(a, ty))
        assert wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p),
                                            P_(lens, wrk._u32p), None, C.byref(run), None, 1) == wrk.E_ARG, field
        q = wrk.QueueOptions()
        pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
        q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
        setattr(q, field, P_(a, ty))
        arrs = [np.zeros(4, np.uint32) for _ in range(5)]
        res = wrk.QueueResult(*[P_(x, wrk._u32p) for x in arrs], C.pointer(run))
        assert wrk.hip.wrk_v7_generate_queue(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1) == wrk.E_ARG, field
    opt = wrk.GenerateOptions()
    opt.window, opt.num_dry_breakers = win.h, 1                                        # a breaker count without the array
    assert wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p),
                                        P_(lens, wrk._u32p), None, C.byref(run), None, 1) == wrk.E_ARG
    assert np.array_equal(bits(rt.state_back(0)), bits(before)), "a refused call launched nothing"
    assert win.back(0).tolist() == [4, 5, 4] and win.back(1).tolist() == []
    # still usable: one program serves another window and other parameters
    zero_states(rt, 2)
    a, _ = rt.generate_greedy([1, 2], 4, window=win, no_repeat_ngram=2)
    w2 = wrk.TokenWindow(ctx, 2, V, 3)
    zero_states(rt, 2)
    b, _ = rt.generate_greedy([1, 2], 4, window=w2, dry=(0.0, 1.75, 2))
    assert w2.back(0).tolist() == b[-3:, 0].tolist() and win.back(1).tolist() == a[:, 1].tolist()
    for h in (w2, foreign, other_ctx, other_vocab, small, win, rt):
        h.close()
