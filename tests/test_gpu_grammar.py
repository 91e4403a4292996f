"""Constrained decoding on the device (web-rwkv-gguf_amd/csrc/wrk_grammar.hip) against the restatement in
tests/grammar_ref.py: the two row functions (`Context.constrain_logits`, `Grammar.advance`), `wrk_grammar_create`'s validation, and a
grammar in every decode loop (`generate_greedy` / `_sample` / `_penalized` / `_stop` / `_queue`) of both runners.

Every comparison is exact: token ids, state words, bit patterns.  The loops run on the tiny fixtures (V = 512), RWKV-7 and RWKV-6,
modes 0 and 1, B in {1, 4} (B = 1 in mode 1 is RWKV-7's persistent engine), RWKV-7 B = 4 also on two lanes.

  identity      a one-state automaton that allows everything changes nothing of any loop (tokens, lengths, logits, log-probs, mu);
  forced chain  an automaton with one way through per start state: every pick family returns exactly the chain, then the end token;
  free choice   a random automaton that allows a third to a half of the vocabulary per state: the tokens are the matching reference pick
                on grammar_ref.mask of the logits of a second runtime that is fed the device's own tokens.  A step is excused only
                where the reference's own ambiguous(...) says so, and at least 95 % of the steps must be checked;
  queue         per-request start and final states, whatever slot and step serve a request."""
import ctypes as C
import functools

import numpy as np
import pytest

import grammar_ref as G
import penalty_ref as R
import wrk
from oracle import synth
from oracle.rnn import stack_cursors

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
# (v6, mode, B, groups)
CONFIGS = [(False, 0, 1, 1), (False, 0, 4, 1), (False, 1, 1, 1), (False, 1, 4, 1), (False, 1, 4, 2), (True, 0, 1, 1), (True, 0, 4, 1),
           (True, 1, 1, 1), (True, 1, 4, 1)]
FIRST = [7, 100, 300, 411]
STEPS = 10
# The seeds are chosen on the CPU: with the oracle's logits in place of the device's, the reference loop of the free-choice test calls
# at most 2 of 60 (B = 1) and 4 of 240 (B = 4) steps ambiguous on either model (a prefix mass within sampling_ref's slack of top_p or
# typical_p: about one step in 25 of a row of some 200 nearly equal tokens, whatever the seed; seeds 21.., 31.. ... 91.. gave 1 to 7 of 60)
SAMPLER = dict(temperature=[0.8, 1.0, 1.3, 0.9], top_p=[0.9, 1.0, 1.0, 0.7], seed=[61, 62, 63, 64])
FAMILIES = {
    "greedy": {},
    "sample": dict(SAMPLER),
    "filter": dict(SAMPLER, top_k=[40, 5, 0, 3], min_p=[0.02, 0.0, 0.1, 0.2]),
    "mirostat": dict(SAMPLER, mirostat=([3.0, 5.0, 0.0, 4.0], [0.1, 0.3, 0.2, 0.05])),
    "typical": dict(SAMPLER, typical_p=[0.9, 0.5, 1.0, 0.7]),
    "pen": dict(SAMPLER, presence=[0.4, 1.5, -0.2, 0.3], frequency=[0.3, 0.0, 0.6, 0.2], decay=[0.996, 1.0, 0.5, 0.9]),
}


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
    return {k: (tuple(x[:B] for x in v) if k == "mirostat" else v[:B]) for k, v in kw.items()}


def run_loop(ctx, rt, family, B, mode, groups, stop=None, occ=None, steps=STEPS, **extra):
    """One call of the loop that belongs to `family` from zero states (penalties: on a zeroed table): everything the call leaves behind."""
    zero_states(rt, B)
    kw = cut(FAMILIES[family], B)
    first = FIRST[:B]
    lens = None
    if family == "pen":
        for b in range(B):
            occ.load(b)
        kw["occurrence"] = occ
    if stop is not None:
        tok, lens, logits = rt.generate_stop(first, steps, stop, mode=mode, groups=groups, want_logits=True, **kw, **extra)
    elif family == "greedy":
        tok, _, logits = rt.generate_greedy(first, steps, mode=mode, groups=groups, want_logits=True, **extra)
    elif family == "pen":
        occurrence = kw.pop("occurrence")
        tok, _, logits = rt.generate_penalized(first, steps, occurrence, mode=mode, groups=groups, want_logits=True, **kw, **extra)
    else:
        tok, _, logits = rt.generate_sample(first, steps, mode=mode, groups=groups, want_logits=True, **kw, **extra)
    return dict(tok=tok, lens=lens, logits=logits, lp=rt.last_logprobs, mu=rt.last_mirostat_mu, gs=rt.last_grammar_state)


# ----------------------------------------------------------------------------- 1. the row functions
def special_rows(rng, n, stride):
    a = rng.normal(0, 3, (n, stride)).astype(np.float32)
    special = np.array([0x7FC00000, 0x7FC01234, 0xFFC00001, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x477FE000, 0xC77FE000,
                        0x00000001, 0x807FFFFF, 0x00800000], np.uint32)
    u = a.view(np.uint32)
    where = rng.random(a.shape) < 0.25
    u[where] = rng.choice(special, int(where.sum()))
    return a


def random_grammar(rng, V, S, NC):
    cls = rng.integers(0, NC, V).astype(np.uint16)
    trans = rng.integers(0, S, (S, NC)).astype(np.uint16)
    trans[rng.random((S, NC)) < 0.5] = G.REJECT
    if NC > 1:
        trans[S - 1, int(cls[0])] = G.REJECT                        # the last state, the one every case uses, rejects something
    used = np.zeros(NC, bool)
    used[cls] = True
    dead = ~((trans != G.REJECT) & used).any(axis=1)
    trans[dead, int(cls[V - 1])] = 0
    return cls, trans


@pytest.mark.parametrize("V", [1, 50, 1023, 1024, 4099, 65536, 70001])
def test_constrain_logits_matches_the_restatement(ctx, V):
    """Both VEC instantiations (V % 4 == 0 with a stride that is a multiple of 4; everything else), the odd tail, and more than one
    workgroup span per row (V > 4096); num_classes 1, 2 and 8192; num_states 1 and 65535 with rows in the last state; in place."""
    rng = np.random.default_rng(V)
    for S_, NC in ((1, 1), (65535, 2), (5, wrk.MAX_TOKEN_CLASSES)):
        cls, trans = random_grammar(rng, V, S_, NC)
        g = wrk.Grammar(ctx, V, cls, trans)
        states = [S_ - 1, 0, S_ // 2, S_ - 1, min(1, S_ - 1)]
        for stride in (V + 8, V + 3):
            a = special_rows(rng, 5, stride)
            buf = ctx.buffer(a)
            assert ctx.constrain_logits(buf, g, states, num_vocab=V, row_stride=stride) is None
            got = buf.read(np.float32, a.size).reshape(5, stride)
            for r in range(5):
                want = G.mask(a[r, :V], cls, trans, states[r])
                assert np.array_equal(bits(got[r, :V]), bits(want)), (S_, NC, stride, r)
                assert np.array_equal(bits(got[r, V:]), bits(a[r, V:])), "the padding between rows is not touched"
        dense = special_rows(rng, 5, V)
        out = ctx.constrain_logits(dense, g, states)
        assert all(np.array_equal(bits(out[r]), bits(G.mask(dense[r], cls, trans, states[r]))) for r in range(5))
        g.close()


def test_advance_matches_the_walk(ctx):
    rng = np.random.default_rng(3)
    V, S_, NC = 4099, 300, 17
    cls, trans = random_grammar(rng, V, S_, NC)
    g = wrk.Grammar(ctx, V, cls, trans)
    assert (g.num_states, g.num_classes, g.num_vocab) == (S_, NC, V)
    states = rng.integers(0, S_, 700).astype(np.uint32)                 # more than one workgroup of rows
    tokens = rng.integers(0, V, 700).astype(np.uint32)
    got = g.advance(states, tokens)
    want = [G.advance(cls, trans, s, t) for s, t in zip(states, tokens)]
    assert got.tolist() == want
    rejected = [i for i in range(700) if trans[states[i], cls[tokens[i]]] == G.REJECT]
    assert len(rejected) > 100 and all(got[i] == states[i] for i in rejected)
    # a walk of several steps, one sequence per row, against Grammar.walk on the host
    s = np.zeros(8, np.uint32)
    seqs = [[] for _ in range(8)]
    for _ in range(12):
        t = [int(rng.choice(np.flatnonzero(G.allowed(cls, trans, int(x))))) for x in s]
        s = g.advance(s, t)
        for b in range(8):
            seqs[b].append(t[b])
    assert [g.walk(0, q) for q in seqs] == s.tolist()
    with pytest.raises(ValueError):
        g.walk(0, [int(np.flatnonzero(~G.allowed(cls, trans, 0))[0])])
    for bad in (lambda: g.advance([S_], [0]), lambda: g.advance([0], [V]), lambda: ctx.constrain_logits(np.zeros((1, V), np.float32), g, [S_])):
        with pytest.raises(wrk.WrkError) as e:
            bad()
        assert e.value.code == wrk.E_ARG
    g.close()


def test_grammar_create_argument_errors(ctx):
    V, S_, NC = 10, 3, 4
    cls = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.uint16)
    trans = np.array([[1, G.REJECT, 2, 0], [G.REJECT, G.REJECT, G.REJECT, 1], [0, 0, 0, 0]], np.uint16)

    def create(V=V, S_=S_, NC=NC, cls=cls, trans=trans):
        h = wrk._P()
        rc = wrk.hip.wrk_grammar_create(ctx.h, V, S_, NC, None if cls is None else P_(cls, wrk._u16p),
                                        None if trans is None else P_(trans, wrk._u16p), C.byref(h))
        if rc == wrk.OK:
            wrk.hip.wrk_grammar_destroy(h)
        else:
            assert not h.value
        return rc

    assert create() == wrk.OK
    assert create(cls=None) == wrk.E_ARG and create(trans=None) == wrk.E_ARG                        # NULL arrays
    c2 = cls.copy()
    c2[7] = NC
    assert create(cls=c2) == wrk.E_ARG                                                              # a class >= num_classes
    t2 = trans.copy()
    t2[1, 2] = S_
    assert create(trans=t2) == wrk.E_ARG                                                            # neither a state nor REJECT
    t3 = trans.copy()
    t3[1, 3] = G.REJECT
    assert create(trans=t3) == wrk.E_ARG                                                            # a state that allows nothing
    c4 = np.where(cls == 3, 0, cls).astype(np.uint16)
    assert create(cls=c4) == wrk.E_ARG                                                              # ... because no token maps to its one class
    assert create(S_=0) == wrk.E_ARG and create(NC=0) == wrk.E_ARG and create(V=0) == wrk.E_ARG
    big = np.zeros((1, wrk.MAX_TOKEN_CLASSES + 1), np.uint16)
    assert create(S_=1, NC=wrk.MAX_TOKEN_CLASSES + 1, trans=big) == wrk.E_ARG
    assert create(S_=65536, trans=np.zeros((65536, NC), np.uint16)) == wrk.E_ARG
    huge = np.zeros(2 ** 20 + 1, np.uint16)
    assert create(V=2 ** 20 + 1, cls=huge) == wrk.E_UNSUPPORTED
    with pytest.raises(ValueError):
        wrk.Grammar(ctx, V + 1, cls, trans)


# ----------------------------------------------------------------------------- 2. identity
def same(a, b, what):
    for k in ("tok", "lens"):
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(bits(a["logits"]), bits(b["logits"])), what
    assert (a["mu"] is None and b["mu"] is None) or np.array_equal(bits(a["mu"]), bits(b["mu"])), what
    n = a["tok"].shape[0] if a["lens"] is None else None
    for x, y in zip(a["lp"], b["lp"]):
        for bb in range(x.shape[1]):
            k = n if n is not None else int(a["lens"][bb])
            assert np.array_equal(x[:k, bb].view(np.uint32), y[:k, bb].view(np.uint32)), (what, "log-probs")


@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_identity_automaton_changes_nothing(ctx, v6, mode, B, groups):
    V = vocab(v6)
    g = wrk.Grammar(ctx, V, np.zeros(V, np.uint16), [[0]])
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    for family in FAMILIES:
        plain = run_loop(ctx, rt, family, B, mode, groups, occ=occ, logprobs=2)
        con = run_loop(ctx, rt, family, B, mode, groups, occ=occ, logprobs=2, grammar=g)
        same(plain, con, family)
        assert plain["gs"] is None and con["gs"].tolist() == [0] * B
        # with stop sets: sequence 0 ends on its fourth token
        stops = [[int(plain["tok"][3, 0])]] + [[] for _ in range(B - 1)]
        plain = run_loop(ctx, rt, family, B, mode, groups, stop=stops, occ=occ, logprobs=2)
        con = run_loop(ctx, rt, family, B, mode, groups, stop=stops, occ=occ, logprobs=2, grammar=g, grammar_state=0)
        assert plain["lens"][0] <= 4
        same(plain, con, family + " with stops")
    # the queue: more requests than slots
    prompts = [[(7 + 13 * r + 29 * i) % V for i in range(n)] for r, n in enumerate([3, 1, 4, 2, 1, 2])]
    for family in ("greedy", "sample", "mirostat", "pen"):
        kw = {k: ((np.resize(v[0], 6), np.resize(v[1], 6)) if k == "mirostat" else np.resize(v, 6)) for k, v in FAMILIES[family].items()}
        if family == "pen":
            kw["occurrence"] = occ
        a, run_a = rt.generate_queue(prompts, max_new=[4, 6, 3, 5, 2, 6], mode=mode, logprobs=2, **kw)
        lp_a, mu_a = rt.last_logprobs, rt.last_mirostat_mu
        b, run_b = rt.generate_queue(prompts, max_new=[4, 6, 3, 5, 2, 6], mode=mode, logprobs=2, grammar=g, **kw)
        assert run_a == run_b and rt.last_grammar_state.tolist() == [0] * 6
        for r in range(6):
            assert a[r][0].tolist() == b[r][0].tolist() and a[r][1:] == b[r][1:], (family, r)
            assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(lp_a[r], rt.last_logprobs[r])), (family, r)
        assert (mu_a is None) or np.array_equal(bits(mu_a), bits(rt.last_mirostat_mu))
    occ.close()
    rt.close()
    g.close()


# ----------------------------------------------------------------------------- 3. forced chain
END = 3
CHAINS = [[500, 17, 250, 9], [501, 44], [502, 8, 8, 8, 130, 131], [503, 511, 0]]


def chain_grammar(ctx, V):
    """One choice per first token: a sequence that starts behind its choice's first token has exactly one way on."""
    cls, trans, start = wrk.grammar_from_choices(V, CHAINS, END)
    g = wrk.Grammar(ctx, V, cls, trans)
    return g, [g.walk(start, c[:1]) for c in CHAINS]


@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_forced_chain(ctx, v6, mode, B, groups):
    V = vocab(v6)
    g, starts = chain_grammar(ctx, V)
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    want = np.array([(c[1:] + [END] * STEPS)[:STEPS] for c in CHAINS[:B]], np.uint32).T
    for family in FAMILIES:
        out = run_loop(ctx, rt, family, B, mode, groups, occ=occ, grammar=g, grammar_state=starts[:B])
        assert np.array_equal(out["tok"], want), family
        assert out["gs"].tolist() == [g.walk(starts[b], want[:, b]) for b in range(B)], family
        out = run_loop(ctx, rt, family, B, mode, groups, occ=occ, stop=[END], grammar=g, grammar_state=starts[:B], poll_steps=2)
        assert out["lens"].tolist() == [len(c) for c in CHAINS[:B]], family               # the chain behind its first token, and END
        for b in range(B):
            n = int(out["lens"][b])
            assert out["tok"][:n, b].tolist() == want[:n, b].tolist(), (family, b)
            assert int(out["gs"][b]) == g.walk(starts[b], out["tok"][:n, b]), "the state froze with the sequence"
    occ.close()
    rt.close()
    g.close()


# ----------------------------------------------------------------------------- 4. free choice
GRAMMAR_SEED = 20


@functools.lru_cache(maxsize=None)
def free_tables(V):
    table = G.random_dense(np.random.default_rng(GRAMMAR_SEED), 6, V, 48)
    share = (table >= 0).mean(axis=1)
    assert share.min() >= 0.3 and share.max() <= 0.55, share
    return wrk.grammar_from_dense(table)


def picks_of(family, B):
    kw = cut(FAMILIES[family], B)
    if family in ("greedy",):
        return [G.Pick("greedy") for _ in range(B)]
    base = [dict(temperature=kw["temperature"][b], top_p=kw["top_p"][b], seed=kw["seed"][b]) for b in range(B)]
    if family == "filter":
        return [G.Pick("filter", top_k=kw["top_k"][b], min_p=kw["min_p"][b], **base[b]) for b in range(B)]
    if family == "mirostat":
        return [G.Pick("mirostat", tau=kw["mirostat"][0][b], eta=kw["mirostat"][1][b], **base[b]) for b in range(B)]
    if family == "typical":
        return [G.Pick("typical", typical_p=kw["typical_p"][b], **base[b]) for b in range(B)]
    return [G.Pick("sample", **base[b]) for b in range(B)]


def replay(ctx, v6, B, mode, family, cls, trans, starts, out):
    """A second runtime is fed the device's own tokens; the reference pick of `family` on grammar_ref.mask of its logits must give the
    device's token wherever the reference does not call the masked row ambiguous.  Returns (steps checked, steps, final states)."""
    V = vocab(v6)
    rt = fresh(ctx, v6, B)
    pk = picks_of(family, B)
    pen = cut(FAMILIES["pen"], B) if family == "pen" else None
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    state = list(starts)
    cur = FIRST[:B]
    checked = total = 0
    for step in range(out["tok"].shape[0]):
        logits = rt.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
        for b in range(B):
            if out["lens"] is not None and step >= out["lens"][b]:
                continue
            y = int(out["tok"][step, b])
            x = logits[b]
            if pen:
                x = R.penalize(x, counts[b], flags[b], pen["presence"][b], pen["frequency"][b])
                counts[b], flags[b] = R.update(counts[b], flags[b], y, ones, pen["decay"][b])
            assert G.allowed(cls, trans, state[b])[y], f"step {step} sequence {b}: token {y} is not allowed in state {state[b]}"
            tok, ambiguous = pk[b].draw(G.mask(x, cls, trans, state[b]), step)
            total += 1
            if not ambiguous:
                assert y == tok, (family, step, b)
                checked += 1
            state[b] = G.advance(cls, trans, state[b], y)
        cur = out["tok"][step].tolist()
    rt.close()
    return checked, total, state


@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_free_choice_matches_the_replay(ctx, v6, mode, B, groups):
    V = vocab(v6)
    cls, trans = free_tables(V)
    g = wrk.Grammar(ctx, V, cls, trans)
    starts = [2, 0, 5, 3][:B]
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    checked = total = 0
    for family in FAMILIES:
        out = run_loop(ctx, rt, family, B, mode, groups, occ=occ, grammar=g, grammar_state=starts)
        c, t, final = replay(ctx, v6, B, mode, family, cls, trans, starts, out)
        print(f"{family}: {c} of {t} steps checked")
        checked, total = checked + c, total + t
        assert out["gs"].tolist() == final == [g.walk(starts[b], out["tok"][:, b]) for b in range(B)], family
        # with a stop set: sequence 0 ends on its fifth token, its state freezes there
        stops = [[int(out["tok"][4, 0])]] + [[] for _ in range(B - 1)]
        cut_ = run_loop(ctx, rt, family, B, mode, groups, occ=occ, stop=stops, grammar=g, grammar_state=starts, poll_steps=2)
        assert cut_["lens"][0] <= 5
        for b in range(B):
            n = int(cut_["lens"][b])
            assert cut_["tok"][:n, b].tolist() == out["tok"][:n, b].tolist(), (family, b)
            assert int(cut_["gs"][b]) == g.walk(starts[b], cut_["tok"][:n, b]), (family, b)
    assert checked >= 0.95 * total, (checked, total)
    occ.close()
    rt.close()
    g.close()


@pytest.mark.parametrize("v6,mode,B", [(False, 1, 1), (False, 1, 4), (True, 1, 4), (False, 0, 4)])
def test_logprobs_stay_on_the_raw_head_output(ctx, v6, mode, B):
    V = vocab(v6)
    cls, trans = free_tables(V)
    g = wrk.Grammar(ctx, V, cls, trans)
    starts = [2, 0, 5, 3][:B]
    rt = fresh(ctx, v6, B)
    out = run_loop(ctx, rt, "sample", B, mode, 1, grammar=g, grammar_state=starts, logprobs=3)
    lp, ids, tlp = out["lp"]
    outside = 0
    state = list(starts)
    for step in range(STEPS):
        # the head output the step's tokens were drawn from: last_logits of the same call cut after that step
        head = run_loop(ctx, rt, "sample", B, mode, 1, steps=step + 1, grammar=g, grammar_state=starts)
        assert np.array_equal(head["tok"], out["tok"][:step + 1])
        want = ctx.top_logprobs(head["logits"], out["tok"][step], 3)
        assert np.array_equal(bits(lp[step]), bits(want[0])) and np.array_equal(ids[step], want[1]) and np.array_equal(bits(tlp[step]), bits(want[2])), step
        for b in range(B):
            outside += int((~G.allowed(cls, trans, state[b])[ids[step, b]]).sum())
            state[b] = G.advance(cls, trans, state[b], int(out["tok"][step, b]))
    assert outside > 0, "no disallowed token among the alternatives: the case shows nothing"
    rt.close()
    g.close()


# ----------------------------------------------------------------------------- 5. the queue
QUEUE_CHAINS = [[400, 17, 250, 9], [401, 44], [402, 8, 8, 8, 130, 131], [403, 511, 0], [404, 1], [405, 6, 7, 8, 9], [406, 2, 2]]
QUEUE_PROMPTS = [3, 1, 5, 2, 4, 1, 2]


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("v6,mode,B", [(False, 1, 1), (False, 1, 2), (False, 0, 3), (True, 1, 2)])
@pytest.mark.parametrize("family", ["greedy", "sample"])
def test_queue_requests_carry_their_own_state(ctx, family, v6, mode, B, pool):
    V = vocab(v6)
    cls, trans, start = wrk.grammar_from_choices(V, QUEUE_CHAINS, END)
    g = wrk.Grammar(ctx, V, cls, trans)
    n = len(QUEUE_CHAINS)
    starts = [g.walk(start, c[:1]) for c in QUEUE_CHAINS]
    prompts = [[(7 + 13 * r + 29 * i) % V for i in range(k)] for r, k in enumerate(QUEUE_PROMPTS)]
    kw = {k: np.resize(v, n) for k, v in FAMILIES[family].items()}
    rt = fresh(ctx, v6, B)
    sp = wrk.StatePool(ctx, rt, n) if pool else None
    pk = dict(pool=sp, save_state=list(range(n))) if pool else {}
    # every reply is its own chain and then END, which ends it (reason 1), whatever slot and step served it: the steps that fed the
    # prompts did not move the states, and a refilled slot did not start in what its previous request left
    got, _ = rt.generate_queue(prompts, stop=[END], max_new=10, mode=mode, poll_steps=4, grammar=g, grammar_state=starts, **kw, **pk)
    for r in range(n):
        assert got[r][0].tolist() == QUEUE_CHAINS[r][1:] + [END] and got[r][1] == 1, r
        assert int(rt.last_grammar_state[r]) == g.walk(starts[r], got[r][0]), r
    assert len({x[2] for x in got}) == B
    # max_steps = 7 cuts the call while, for every B here, one request is running (reason 3: the state reached so far, the start state
    # while it is still feeding its prompt) and others were never dispatched (reason 0: the entry is untouched); at B = 3 request 2 has
    # been cut short by max_new before that (reason 2: the state it reached)
    got, run = rt.generate_queue(prompts, stop=[END], max_new=[10, 10, 3, 10, 10, 10, 10], max_steps=7, mode=mode, poll_steps=4, grammar=g,
                                 grammar_state=starts, **kw, **pk)
    reasons = [x[1] for x in got]
    assert 3 in reasons and 0 in reasons and (B < 3 or reasons[2] == 2), reasons
    for r in range(n):
        assert got[r][0].tolist() == (QUEUE_CHAINS[r][1:] + [END])[:len(got[r][0])], r
        assert int(rt.last_grammar_state[r]) == g.walk(starts[r], got[r][0]), (r, reasons[r])
    if sp:
        sp.close()
    rt.close()
    g.close()


# ----------------------------------------------------------------------------- 6. argument errors
def test_argument_errors_leave_the_model_usable(ctx):
    V = vocab()
    rt = fresh(ctx, False, 2)
    cls, trans = free_tables(V)
    g = wrk.Grammar(ctx, V, cls, trans)
    other = wrk.Grammar(ctx, V + 1, np.zeros(V + 1, np.uint16), [[0]])
    rt.generate_greedy([1, 2], 3)
    before = rt.state_back(0).copy()
    for kw in (dict(grammar=g, grammar_state=[0, 6]), dict(grammar=g, grammar_state=2 ** 32 - 1), dict(grammar=other)):
        for call in (lambda: rt.generate_greedy([1, 2], 3, **kw), lambda: rt.generate_sample([1, 2], 3, **kw),
                     lambda: rt.generate_stop([1, 2], 3, [5], **kw), lambda: rt.generate_queue([[1, 2], [3]], max_new=2, **kw)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, kw
    with pytest.raises(ValueError):
        rt.generate_greedy([1, 2], 3, grammar_state=[0, 0])
    # grammar_state without a grammar, through the ABI
    ft, st = np.array([1, 2], np.uint32), np.zeros(2, np.uint32)
    out, lens, run = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32), C.c_uint32()
    opt = wrk.GenerateOptions()
    opt.grammar_state = P_(st, wrk._u32p)
    assert wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p), P_(lens, wrk._u32p),
                                        None, C.byref(run), None, 1) == wrk.E_ARG
    q = wrk.QueueOptions()
    pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
    q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
    q.grammar_state = P_(st, wrk._u32p)
    arrs = [np.zeros(4, np.uint32) for _ in range(5)]
    res = wrk.QueueResult(*[P_(a, wrk._u32p) for a in arrs], C.pointer(run))
    assert wrk.hip.wrk_v7_generate_queue(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1) == wrk.E_ARG
    assert np.array_equal(bits(rt.state_back(0)), bits(before)), "a refused call launched nothing"
    # still usable: the greedy loop from a zero state equals a fresh runtime's, and a constrained call runs
    zero_states(rt, 2)
    t, _ = rt.generate_greedy([1, 2], 4)
    fresh_rt = fresh(ctx, False, 2)
    assert np.array_equal(t, fresh_rt.generate_greedy([1, 2], 4)[0])
    fresh_rt.close()
    t, _ = rt.generate_greedy([1, 2], 4, grammar=g, grammar_state=[1, 4])
    assert rt.last_grammar_state.tolist() == [g.walk(1, t[:, 0]), g.walk(4, t[:, 1])]
    rt.close()
    other.close()
    g.close()


def test_one_program_serves_any_grammar_and_any_start_states(ctx):
    """The tables and the states are device data: a second grammar and other start states replay the program the first call captured
    (the call would otherwise still follow the first grammar), and calls without a grammar are unaffected in between."""
    V = vocab()
    rt = fresh(ctx, False, 2)
    plain, _ = rt.generate_greedy(FIRST[:2], 6)
    g1, s1 = chain_grammar(ctx, V)
    cls, trans, start = wrk.grammar_from_choices(V, [[9, 8, 7, 6], [5, 4]], 2)
    g2 = wrk.Grammar(ctx, V, cls, trans)
    for _ in range(2):
        zero_states(rt, 2)
        a, _ = rt.generate_greedy(FIRST[:2], 6, grammar=g1, grammar_state=s1[:2])
        assert a.T.tolist() == [(c[1:] + [END] * 6)[:6] for c in CHAINS[:2]]
        zero_states(rt, 2)
        b, _ = rt.generate_greedy(FIRST[:2], 6, grammar=g2, grammar_state=[g2.walk(start, [9]), g2.walk(start, [5])])
        assert b.T.tolist() == [[8, 7, 6, 2, 2, 2], [4, 2, 2, 2, 2, 2]]
        zero_states(rt, 2)
        assert np.array_equal(rt.generate_greedy(FIRST[:2], 6)[0], plain)
    rt.close()
    g1.close()
    g2.close()
