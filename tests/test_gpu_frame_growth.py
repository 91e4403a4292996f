"""Growth of a frame's side buffers under cached step programs (web-rwkv-gguf_amd/csrc/wrk_dev_group.h).

A step program holds the addresses of the frame's buffer groups.  When a larger call makes a group reallocate, the programs of the
frame must go with the old memory: a program that survived would read freed memory.  Every case makes three calls in a row on one
`Runtime` -- a small one, a large one that grows the groups, and the small one again, whose program key existed before the buffers
moved -- and compares everything each call returns, bit for bit, with the same call on a fresh `Runtime`.

The calls turn on everything that owns a group: a sampler with an occurrence table, top-k or Mirostat, log-probs, an accept-all
grammar of one state, stop ids and stop sequences (taken from what the call draws without stops, so that sequences do end and are
frozen and restored), and in the queue the request tables and, with a `StatePool`, the pool's.  `small` synthetic models (V = 1000),
num_batch = 4."""
import functools

import numpy as np
import pytest

import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

NB = 4
SAMPLER = dict(temperature=[1.0, 0.8, 1.2, 0.9], top_p=[0.9, 1.0, 0.8, 0.95])
PEN = dict(presence=0.3, frequency=0.2, decay=0.996)
PICKS = {"top_k": dict(top_k=[40, 5, 200, 17]), "mirostat": dict(mirostat=(3.0, 0.1))}
STOP_SHAPES = [(2, 4), (4, 12), (2, 4)]         # (sequences, steps): small, large, small again
QUEUE_SHAPES = [3, 9, 3]                        # requests


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(v6):
    return synth.make_v6_gguf(synth.V6_CONFIGS["small"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["small"], 42)


def vocab(v6):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)["small"].num_vocab


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    """got == want, bit for bit, through dicts, lists and tuples"""
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        for k in want:
            same(got[k], want[k], f"{what}.{k}")
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, f"{what}[{i}]")
    elif want is None or isinstance(want, (bool, int)):
        assert got == want, what
    else:
        g, w = bits(got), bits(want)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), what


def rows(pick, n):
    """the per-row sampler arguments of n sequences or requests"""
    kw = {k: [v[i % 4] for i in range(n)] for k, v in SAMPLER.items()} | {"seed": [11 + i for i in range(n)]} | PEN
    return kw | {k: ([v[i % 4] for i in range(n)] if isinstance(v, list) else v) for k, v in PICKS[pick].items()}


class Bench:
    """One `Runtime` of NB slots; every call starts from zero states, a fresh occurrence table and a fresh accept-all grammar."""

    def __init__(self, ctx, v6):
        self.ctx, self.v6, self.V = ctx, v6, vocab(v6)
        self.rt = wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=NB)
        self.zero = np.zeros_like(self.rt.state_back(0))

    def close(self):
        self.rt.close()

    def _fresh(self):
        for b in range(NB):
            self.rt.state_load(self.zero, b)
        occ = wrk.Occurrence(self.ctx, NB, self.V)
        for b in range(NB):
            occ.load(b)
        return occ, wrk.Grammar(self.ctx, self.V, np.zeros(self.V, np.uint16), [[0]])

    def stop(self, pick, B, steps, groups, stop, seqs):
        """generate_stop of B sequences; stop / seqs None: the call without stops, for choosing them"""
        rt = self.rt
        occ, g = self._fresh()
        first = [3 + 7 * b for b in range(B)]
        probe = stop is None
        tok, lens, logits = rt.generate_stop(first, steps, [] if probe else stop, occurrence=occ, groups=groups, want_logits=True, poll_steps=4,
                                             logprobs=None if probe else 2, grammar=g, stop_sequences=seqs, **rows(pick, B))
        cp = lambda a: None if a is None else np.array(a)
        out = dict(tok=tok, lens=lens, logits=logits, lp=rt.last_logprobs, mu=cp(rt.last_mirostat_mu), gs=cp(rt.last_grammar_state),
                   match=cp(rt.last_stop_match), tail=cp(rt.last_stop_tail), state=[rt.state_back(b) for b in range(B)],
                   occ=[occ.back(b) for b in range(B)])
        occ.close()
        g.close()
        return out

    def queue(self, pick, R, pool, stop, seqs):
        """generate_queue of R requests on the NB slots; with `pool` every request starts from and saves to an entry of its own"""
        rt = self.rt
        occ, g = self._fresh()
        prompts = [[5 + 3 * r, 9 + r] + ([21 + r] if r % 2 else []) for r in range(R)]
        probe = stop is None
        sp = wrk.StatePool(self.ctx, rt, R) if pool else None
        kw = dict(pool=sp, start_state=list(range(R)), save_state=list(range(R))) if pool else {}
        res, run = rt.generate_queue(prompts, stop=[] if probe else stop, max_new=[5 + r % 3 for r in range(R)], occurrence=occ, poll_steps=4,
                                     logprobs=None if probe else 2, grammar=g, stop_sequences=seqs, **rows(pick, R), **kw)
        cp = lambda a: None if a is None else np.array(a)
        out = dict(res=[(t, [reason, slot, start]) for t, reason, slot, start in res], run=run, lp=rt.last_logprobs, mu=cp(rt.last_mirostat_mu),
                   gs=cp(rt.last_grammar_state), match=cp(rt.last_stop_match), saved=rt.last_queue_saved,
                   entries=[sp.back(k) for k in range(R)] if pool else None)
        if sp:
            sp.close()
        occ.close()
        g.close()
        return out


def stops_of(draws):
    """Stops for owners whose draws without stops are `draws` (one id list each): owner 0 ends on the id of its third draw, owner 1 on
    the stop sequence of its second and third; the others have neither."""
    n = len(draws)
    stop, seqs = [[] for _ in range(n)], [[] for _ in range(n)]
    stop[0] = [int(draws[0][2])]
    seqs[1] = [[int(draws[1][1]), int(draws[1][2])]]
    return stop, seqs


class Fresh:
    """What fresh runtimes return, computed once per call and shared by the cases (never changed afterwards)."""

    def __init__(self, ctx):
        self.ctx, self.memo = ctx, {}

    def _on_fresh(self, v6, fn):
        b = Bench(self.ctx, v6)
        try:
            return fn(b)
        finally:
            b.close()

    def stop(self, v6, pick, B, steps, groups):
        """(stop, seqs, result) of the stop call"""
        key = ("stop", v6, pick, B, steps, groups)
        if key not in self.memo:
            tok = self._on_fresh(v6, lambda b: b.stop(pick, B, steps, groups, None, None))["tok"]
            stop, seqs = stops_of([tok[:, b] for b in range(B)])
            self.memo[key] = (stop, seqs, self._on_fresh(v6, lambda b: b.stop(pick, B, steps, groups, stop, seqs)))
        return self.memo[key]

    def queue(self, v6, pick, R, pool):
        key = ("queue", v6, pick, R, pool)
        if key not in self.memo:
            probe = ("probe", v6, pick, R)
            if probe not in self.memo:      # the replies without stops do not depend on the pool: every entry starts as zeros
                res = self._on_fresh(v6, lambda b: b.queue(pick, R, False, None, None))["res"]
                self.memo[probe] = stops_of([t for t, _ in res])
            stop, seqs = self.memo[probe]
            self.memo[key] = (stop, seqs, self._on_fresh(v6, lambda b: b.queue(pick, R, pool, stop, seqs)))
        return self.memo[key]


@pytest.fixture(scope="module")
def fresh(ctx):
    return Fresh(ctx)


@pytest.mark.parametrize("v6,pick,groups", [(False, "top_k", 1), (False, "mirostat", 1), (False, "top_k", 2), (True, "top_k", 1), (True, "mirostat", 1)])
def test_stop_calls_across_growth(ctx, fresh, v6, pick, groups):
    b = Bench(ctx, v6)
    try:
        for i, (B, steps) in enumerate(STOP_SHAPES):
            stop, seqs, want = fresh.stop(v6, pick, B, steps, groups)
            assert int(want["lens"][0]) <= 3 and int(want["lens"][1]) <= 3 and want["tok"].shape[1] == B       # the stops do end sequences
            same(b.stop(pick, B, steps, groups, stop, seqs), want, f"call {i} ({B} sequences, {steps} steps)")
    finally:
        b.close()


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("v6,pick", [(False, "top_k"), (False, "mirostat"), (True, "top_k"), (True, "mirostat")])
def test_queue_calls_across_growth(ctx, fresh, v6, pick, pool):
    b = Bench(ctx, v6)
    try:
        for i, R in enumerate(QUEUE_SHAPES):
            stop, seqs, want = fresh.queue(v6, pick, R, pool)
            assert want["res"][0][1][0] == 1 and want["res"][1][1][0] == 1 and len(want["res"]) == R            # both stops ended their requests
            same(b.queue(pick, R, pool, stop, seqs), want, f"call {i} ({R} requests)")
    finally:
        b.close()
