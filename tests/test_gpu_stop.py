"""Stop tokens in the decode loops (web-rwkv-gguf_amd/csrc/wrk_stop.hip) through `Runtime.generate_stop`, against the
restatement in tests/stop_ref.py and against calls without stops: tokens, lengths, frozen state / occurrence slot / logits row, early
exit, continuation and host validation.

The stop ids come from what the same call draws without stops (a token that does not occur earlier in its sequence), so a stopped run
must end exactly there."""
import ctypes as C

import numpy as np
import pytest

import penalty_ref as P
import stop_ref as R
import wrk
from oracle import synth

pytestmark = pytest.mark.gpu

SAMPLER = dict(temperature=[1.0, 0.8, 1.2, 0.9], top_p=[0.9, 1.0, 0.8, 0.95])
PEN = dict(presence=0.3, frequency=0.2, decay=0.996)


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def model(cfg="small", v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS[cfg], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS[cfg], 42)


def vocab(cfg="small", v6=False):
    return (synth.V6_CONFIGS if v6 else synth.CONFIGS)[cfg].num_vocab


def first_tokens(B, V):
    return [(5 + 61 * b) % V for b in range(B)]


def sampler(B):
    return {k: [v[b % 4] for b in range(B)] for k, v in SAMPLER.items()} | {"seed": [11 + b for b in range(B)]}


class Run:
    """One call on a fresh runtime (zero state, zero occurrence table): kind greedy / sample / pen, with or without stop sets."""

    def __init__(self, ctx, data, V, B, kind, mode, groups, steps, first=None, stop=None, poll_steps=0, ban=None, load_state=None):
        rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
        occ = wrk.Occurrence(ctx, B, V) if kind == "pen" else None
        for b, ids in (ban or {}).items():
            occ.ban(b, ids)
        for b, s in enumerate(load_state or []):
            rt.state_load(s, b)
        first = first_tokens(B, V) if first is None else first
        kw = {} if kind == "greedy" else sampler(B)
        if stop is None:
            if kind == "greedy":
                self.tokens, _, self.logits = rt.generate_greedy(first, steps, mode=mode, want_logits=True, groups=groups)
            elif kind == "sample":
                self.tokens, _, self.logits = rt.generate_sample(first, steps, mode=mode, want_logits=True, groups=groups, **kw)
            else:
                self.tokens, _, self.logits = rt.generate_penalized(first, steps, occ, mode=mode, want_logits=True, groups=groups, **kw, **PEN)
            self.lengths = np.full(B, steps, np.uint32)
        else:
            pk = dict(occurrence=occ, **PEN) if kind == "pen" else {}
            self.tokens, self.lengths, self.logits = rt.generate_stop(first, steps, stop, mode=mode, want_logits=True, groups=groups,
                                                                      poll_steps=poll_steps, **kw, **pk)
        self.state = [rt.state_back(b) for b in range(B)]
        self.occ = [occ.back(b) for b in range(B)] if occ else None
        if occ:
            occ.close()
        rt.close()


def new_at(tokens, b, k):
    """(step j >= k, id): the first token of sequence b at or after step k that does not occur earlier in the sequence."""
    col = tokens[:, b].tolist()
    for j in range(k, len(col)):
        if col[j] not in col[:j]:
            return j, col[j]
    raise AssertionError(f"sequence {b} draws no new token from step {k} on: {col}")


def last_new(tokens, b):
    col = tokens[:, b].tolist()
    for j in range(len(col) - 1, -1, -1):
        if col[j] not in col[:j]:
            return j, col[j]


def unused_id(tokens, V):
    return next(i for i in range(V - 1, -1, -1) if i not in set(tokens.reshape(-1).tolist()))


def check_against_plain(ctx, data, V, B, kind, mode, groups, steps, plain, got, stops):
    """tokens / lengths against stop_ref, then state, logits row and occurrence slot of every sequence against the call without stops
    that runs lengths[b] steps (one such call per distinct length; same B, mode and lanes)."""
    want_tokens, want_len = R.apply(plain.tokens[:steps], stops, steps_run=got.tokens.shape[0])
    assert got.lengths.tolist() == want_len.tolist()
    assert np.array_equal(got.tokens, want_tokens)
    refs = {}
    for b in range(B):
        n = int(got.lengths[b])
        if n not in refs:
            refs[n] = plain if n == plain.tokens.shape[0] else Run(ctx, data, V, B, kind, mode, groups, n)
        ref = refs[n]
        assert np.array_equal(ref.tokens[:, b], got.tokens[:n, b]), b
        assert np.array_equal(bits(got.state[b]), bits(ref.state[b])), f"state of sequence {b} (length {n})"
        assert np.array_equal(bits(got.logits[b]), bits(ref.logits[b])), f"last logits of sequence {b} (length {n})"
        if kind == "pen":
            c, f = got.occ[b]
            wc, wf = P.update_all(np.zeros(V, np.float32), np.zeros(V, np.uint32), got.tokens[:n, b], np.ones(V, np.float32), PEN["decay"])
            assert np.array_equal(bits(c), bits(wc)) and np.array_equal(f, wf), f"occurrence slot {b}"
            assert np.array_equal(bits(c), bits(ref.occ[b][0])) and np.array_equal(f, ref.occ[b][1]), b
    return refs


# ----------------------------------------------------------------------------------------------------------------- 1. empty stop sets
@pytest.mark.parametrize("kind", ["greedy", "sample", "pen"])
@pytest.mark.parametrize("mode,v6", [(0, False), (1, False), (1, True)])
def test_empty_stop_sets_are_the_plain_call(ctx, mode, v6, kind):
    data, V, B, steps = model("small", v6), vocab("small", v6), 3, 12
    plain = Run(ctx, data, V, B, kind, mode, 1, steps)
    for stop in ([], [[] for _ in range(B)]):
        got = Run(ctx, data, V, B, kind, mode, 1, steps, stop=stop)
        assert got.tokens.shape == (steps, B) and got.lengths.tolist() == [steps] * B
        assert np.array_equal(got.tokens, plain.tokens)
        assert np.array_equal(bits(got.logits), bits(plain.logits))
        for b in range(B):
            assert np.array_equal(bits(got.state[b]), bits(plain.state[b])), b
            if kind == "pen":
                assert np.array_equal(bits(got.occ[b][0]), bits(plain.occ[b][0])) and np.array_equal(got.occ[b][1], plain.occ[b][1]), b


# ----------------------------------------------------------------------------------------------------------------- 2, 3, 4, 5
#          B  mode groups v6  eager engine kind
SHAPES = [(1, 1, 1, False, None, None, "greedy"),       # batch-1 engine
          (1, 1, 1, False, None, "0", "sample"),        # five-launch layer
          (1, 0, 1, False, None, None, "sample"),
          (3, 0, 1, False, None, None, "sample"),
          (3, 1, 1, False, None, None, "greedy"),
          (3, 1, 1, False, None, None, "pen"),
          (16, 1, 1, False, None, None, "sample"),
          (16, 0, 1, False, None, None, "greedy"),
          (3, 1, 1, False, "1", None, "sample"),        # WRK_NO_GRAPH=1
          (3, 0, 1, False, "1", None, "pen"),
          (4, 1, 2, False, None, None, "pen"),          # two lanes
          (4, 1, 2, False, None, None, "greedy"),
          (3, 1, 1, True, None, None, "sample"),
          (3, 0, 1, True, None, None, "pen"),
          (3, 1, 1, True, "1", None, "greedy")]


@pytest.mark.parametrize("B,mode,groups,v6,eager,engine,kind", SHAPES)
def test_prefix_padding_and_frozen_slots(ctx, monkeypatch, B, mode, groups, v6, eager, engine, kind):
    if eager is not None:
        monkeypatch.setenv("WRK_NO_GRAPH", eager)
    if engine is not None:
        monkeypatch.setenv("WRK_ENGINE", engine)
    data, V, steps = model("small", v6), vocab("small", v6), 20
    plain = Run(ctx, data, V, B, kind, mode, groups, steps)
    spare = unused_id(plain.tokens, V)
    # where sequences end: step 0, mid-run (two stop ids, one never drawn), the last step; the others never end
    ends = {0: new_at(plain.tokens, 0, 0), 1: new_at(plain.tokens, min(1, B - 1), 5), 2: last_new(plain.tokens, min(2, B - 1))}
    if B == 1:
        scenarios = [[[ends[0][1]]], [[spare, ends[1][1]]], [[ends[2][1]]]]
        run_steps = [steps, steps, ends[2][0] + 1]
    else:
        stops = [[] for _ in range(B)]
        stops[0] = [ends[0][1]]
        stops[1] = [spare, ends[1][1]]
        scenarios = [stops, [list(s) for s in stops]]
        scenarios[1][2] = [ends[2][1]]                  # a second scenario that ends on its own last step
        run_steps = [steps, ends[2][0] + 1]
    for stop, n in zip(scenarios, run_steps):
        got = Run(ctx, data, V, B, kind, mode, groups, n, stop=stop, poll_steps=4)
        assert got.tokens.shape[0] <= n
        check_against_plain(ctx, data, V, B, kind, mode, groups, n, plain if n == steps else Run(ctx, data, V, B, kind, mode, groups, n),
                            got, stop)
    assert plain.tokens.shape[0] == steps


def test_banned_stop_token_never_ends_the_sequence(ctx):
    data, V, B, steps = model("small"), vocab("small"), 3, 16
    plain = Run(ctx, data, V, B, "pen", 1, 1, steps)
    j, tok = new_at(plain.tokens, 1, 4)
    banned = Run(ctx, data, V, B, "pen", 1, 1, steps, ban={1: [tok]})                        # the reference: the same ban, no stops
    got = Run(ctx, data, V, B, "pen", 1, 1, steps, stop=[[], [tok], []], ban={1: [tok]})
    assert tok not in banned.tokens[:, 1].tolist()
    assert got.lengths.tolist() == [steps] * B and got.tokens.shape[0] == steps
    assert np.array_equal(got.tokens, banned.tokens)
    for b in range(B):
        assert np.array_equal(bits(got.state[b]), bits(banned.state[b]))
        assert np.array_equal(bits(got.occ[b][0]), bits(banned.occ[b][0])) and np.array_equal(got.occ[b][1], banned.occ[b][1])


# ----------------------------------------------------------------------------------------------------------------- 6. early exit
@pytest.mark.parametrize("groups", [1, 2])
def test_early_exit(ctx, groups):
    data, V, B, steps, poll = model("small"), vocab("small"), 4, 2048, 8
    plain = Run(ctx, data, V, B, "sample", 1, groups, 128)
    ends = [new_at(plain.tokens, b, 3 + 9 * b) for b in range(B)]
    assert max(j for j, _ in ends) < 64
    stops = [[t] for _, t in ends]
    got = Run(ctx, data, V, B, "sample", 1, groups, steps, stop=stops, poll_steps=poll)
    run = got.tokens.shape[0]
    print(f"early exit: lengths {got.lengths.tolist()}, steps_run {run}, bound {R.steps_run_bound(got.lengths, poll, steps)}")
    assert got.lengths.tolist() == [j + 1 for j, _ in ends]
    assert run <= R.steps_run_bound(got.lengths, poll, steps)
    assert run >= int(got.lengths.max())
    want, _ = R.apply(plain.tokens, stops, steps_run=run)
    assert np.array_equal(got.tokens, want)
    # one sequence that cannot end: every step runs
    stops[2] = []
    got = Run(ctx, data, V, B, "sample", 1, groups, steps, stop=stops, poll_steps=poll)
    assert got.tokens.shape[0] == steps
    assert got.lengths.tolist() == [ends[0][0] + 1, ends[1][0] + 1, steps, ends[3][0] + 1]


# ----------------------------------------------------------------------------------------------------------------- 7. continuation
@pytest.mark.parametrize("v6", [False, True])
def test_continuation_from_the_frozen_state(ctx, v6):
    data, V, B, steps = model("small", v6), vocab("small", v6), 3, 16
    plain = Run(ctx, data, V, B, "sample", 1, 1, steps)
    stops = [[new_at(plain.tokens, 0, 2)[1]], [], [new_at(plain.tokens, 2, 7)[1]]]
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    kw = sampler(B)
    tok, lens = rt.generate_stop(first_tokens(B, V), steps, stops, mode=1, **kw)
    nxt = [int(tok[lens[b] - 1, b]) for b in range(B)]              # the stop token is drawn, not consumed: it is fed next
    second, lens2 = rt.generate_stop(nxt, 10, [[], [], []], mode=1, **kw)
    rt.close()
    # the reference: every slot loaded with the state of the call without stops that runs lengths[b] steps
    ref_state = [Run(ctx, data, V, B, "sample", 1, 1, int(lens[b])).state[b] for b in range(B)]
    want = Run(ctx, data, V, B, "sample", 1, 1, 10, first=nxt, stop=[[], [], []], load_state=ref_state)
    assert lens.tolist() == R.lengths(plain.tokens, stops).tolist()
    assert np.array_equal(second, want.tokens) and lens2.tolist() == [10] * B


# ----------------------------------------------------------------------------------------------------------------- 8. one program
def test_one_program_serves_any_stop_sets(ctx):
    data, V, B, steps = model("small"), vocab("small"), 3, 16
    plain = Run(ctx, data, V, B, "greedy", 1, 1, steps)
    zero = np.zeros_like(plain.state[0])
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    first = first_tokens(B, V)

    def reset():
        for b in range(B):
            rt.state_load(zero, b)
    before, _ = rt.generate_greedy(first, steps, mode=1)
    for stops in ([[new_at(plain.tokens, 0, 1)[1]], [], []], [[], [new_at(plain.tokens, 1, 0)[1]], [new_at(plain.tokens, 2, 6)[1]]]):
        reset()
        tok, lens = rt.generate_stop(first, steps, stops, mode=1)
        want, wl = R.apply(plain.tokens, stops, steps_run=tok.shape[0])
        assert np.array_equal(tok, want) and lens.tolist() == wl.tolist()
    reset()
    after, _ = rt.generate_greedy(first, steps, mode=1)
    rt.close()
    assert np.array_equal(before, plain.tokens) and np.array_equal(after, plain.tokens)


# ----------------------------------------------------------------------------------------------------------------- 9. validation
@pytest.mark.parametrize("v6", [False, True])
def test_bad_arguments_are_rejected_before_any_launch(ctx, v6):
    data, V, B, steps = model("tiny", v6), vocab("tiny", v6), 2, 6
    rt = wrk.Runtime(ctx, wrk.GgufReader(data), num_batch=B)
    occ = wrk.Occurrence(ctx, B, V)
    rt.generate_greedy([3, 4], 5)                                   # a state that is not zero
    state = [rt.state_back(b) for b in range(B)]
    for stop in ([list(range(wrk.MAX_STOP_TOKENS + 1)), []], [[V], []], [[1], [2, V + 7]]):
        with pytest.raises(wrk.WrkError):
            rt.generate_stop([3, 4], steps, stop)
    with pytest.raises(wrk.WrkError):
        rt.generate_stop([3, V], steps, [])                         # what generate_greedy rejects
    with pytest.raises(wrk.WrkError):
        rt.generate_stop([3, 4], steps, [], temperature=-1.0)       # what generate_sample rejects
    with pytest.raises(wrk.WrkError):
        rt.generate_stop([3, 4], steps, [], occurrence=occ, decay=1.5)      # what generate_penalized rejects

    # the cases the Python wrapper cannot express, through the C ABI
    fn, mdl = (wrk.hip.wrk_v6_generate_stop, rt.model6) if v6 else (wrk.hip.wrk_v7_generate_stop, rt.model)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    ft = np.array([3, 4], np.uint32)
    out, lens, run = np.zeros((steps, B), np.uint32), np.zeros(B, np.uint32), C.c_uint32()
    ids = np.array([1, 2, 3], np.uint32)
    t = np.ones(B, np.float32)
    sd = np.zeros(B, np.uint32)

    def call(opt, lengths=lens):
        return fn(ctx.h, mdl, rt.state, ft.ctypes.data_as(u32p), B, steps, C.byref(opt) if opt is not None else None, out.ctypes.data_as(u32p),
                  lengths.ctypes.data_as(u32p) if lengths is not None else None, None, C.byref(run), None, 1)

    def options(offsets=(0, 1, 3), **kw):
        o = wrk.GenerateOptions()
        off = np.array(offsets, np.uint32)
        o.stop_tokens, o.stop_offsets = ids.ctypes.data_as(u32p), off.ctypes.data_as(u32p)
        for k, v in kw.items():
            setattr(o, k, v.ctypes.data_as(u32p if v.dtype == np.uint32 else f32p))
        o._keep = off
        return o
    assert call(options()) == 0                                     # the well-formed call the bad ones are variations of
    for b in range(B):
        rt.state_load(state[b], b)
    bad = [call(None), call(options(), lengths=None), call(options(offsets=(1, 2, 3))), call(options(offsets=(0, 2, 1))),
           call(options(temperature=t)), call(options(temperature=t, top_p=t)), call(options(top_p=t, seed=sd)),
           call(options(presence=t))]
    assert bad == [1] * len(bad), bad                               # WRK_E_ARG
    for b in range(B):
        assert np.array_equal(bits(rt.state_back(b)), bits(state[b])), b
    occ.close()
    rt.close()
