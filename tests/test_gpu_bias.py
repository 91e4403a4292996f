"""Logit bias on the device (web-rwkv-gguf_amd/csrc/wrk_bias.hip) against the restatement in tests/bias_ref.py: the row
function (`Context.bias_logits`), `wrk_logit_bias_create`'s and the options' validation, and a bias in every decode loop
(`generate_greedy` / `_sample` / `_penalized` / `_stop` / `_queue`) of both runners.

Every comparison is exact: token ids and bit patterns.  The loops run on the tiny fixtures (V = 512), RWKV-7 and RWKV-6, modes 0 and
1, B in {1, 4} (B = 1 in mode 1 is RWKV-7's persistent engine), RWKV-7 B = 4 also on two lanes -- the configurations, pick families,
first tokens and sampler parameters of tests/test_gpu_grammar.py.

  identity     an empty set and WRK_BIAS_NONE change nothing of any loop (tokens, lengths, logits, log-probs, mu);
  forced       a set {t_b: 1e30} makes every step of every family return t_b;
  bans         bias bans against the occurrence table's bans, and against a one-state automaton, device against device;
  replay       per sequence a random set (sizes 64, 1, 200, 17; values uniform in [-4, 4], a quarter of them -inf) from
               np.random.default_rng(REPLAY_SEED[v6]): the tokens are the matching reference pick on bias_ref.apply of the logits of a
               second runtime that is fed the device's own tokens, penalised through penalty_ref for that family.  A step is excused
               only where the reference's own ambiguous(...) says so (greedy: never), and at least 95 % of the steps, summed over the
               six families, must be checked.  The seeds are chosen on the CPU: with the oracle's logits in place of the device's and
               the sets of replay_sets below, the reference loop calls 1 of 60 (B = 1) and 3 of 240 (B = 4) steps ambiguous on RWKV-7
               with seed 157, and 1 of 60 and 5 of 240 on RWKV-6 with seed 47 (a prefix mass within sampling_ref's slack of top_p or
               typical_p; of the seeds 1 .. 160 few stay at or below 2 of 60 and 6 of 240 on either model), and the bias changes 37
               (RWKV-7) and 30 (RWKV-6) of the 40 greedy picks at B = 4, all 10 of sequence 0's on both, so a kernel that does
               nothing fails in every configuration.  Every configuration replays all six families and asserts every step the
               reference does not excuse.  The 95 % bar is one for 240 steps and is asked where four sequences run: at B = 1 only
               set 0 runs, on 60 steps of which the reference excuses about one in 25 for sequence 0's parameters whatever the seed,
               and three excused steps already miss it;
  queue        every request with its own set, whatever slot and step serve it, host dispatch against device dispatch."""
import ctypes as C
import functools

import numpy as np
import pytest

import bias_ref as BR
import grammar_ref as G
import penalty_ref as R
import test_gpu_grammar as TG
import wrk
from oracle.rnn import stack_cursors

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
CONFIGS, FAMILIES, FIRST, STEPS = TG.CONFIGS, TG.FAMILIES, TG.FIRST, TG.STEPS
bits, vocab, fresh, zero_states, run_loop, same = TG.bits, TG.vocab, TG.fresh, TG.zero_states, TG.run_loop, TG.same
NONE = wrk.BIAS_NONE
INF = np.float32(np.inf)
SPAN, TILE = 4096, 1024         # BIAS_SPAN, BIAS_TILE of wrk_bias.hip


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


# ----------------------------------------------------------------------------- 1. the row function
def row_sets(rng, V):
    """[empty, one entry, mixed, dense]: the mixed set has ids 0, V - 1 and both sides of every tile boundary, finite values and bans;
    the dense one has V - 1 entries (every token but one), a third of them bans."""
    edge = {0, V - 1}
    for a in range(TILE, V, TILE):
        edge |= {a - 1, a}
    edge |= set(rng.choice(V, min(V, 40), replace=False).tolist())
    mixed = np.array(sorted(edge), np.int64)
    mixed = mixed[rng.permutation(mixed.size)]                                  # the caller's order is not sorted
    mv = rng.uniform(-8, 8, mixed.size).astype(np.float32)
    mv[rng.random(mixed.size) < 0.3] = -INF
    if (mv == -INF).sum() >= V:
        mv[0] = 0.5                                                             # a set may not ban the whole vocabulary
    dense = rng.permutation(V)[:max(V - 1, 0)]
    dv = rng.uniform(-8, 8, dense.size).astype(np.float32)
    dv[rng.random(dense.size) < 0.33] = -INF
    one = (np.array([V - 1]), np.array([-INF if V > 1 else 1.25], np.float32))
    return [(np.zeros(0, np.int64), np.zeros(0, np.float32)), one, (mixed, mv), (dense, dv)]


@pytest.mark.parametrize("V", [1, 3, 50, 1023, 1024, 1025, 4099, 65536, 70001, 2 ** 20])
def test_bias_logits_matches_the_restatement(ctx, V):
    """Five rows per call with the sets NONE, empty, one entry, mixed and dense; tight rows and a stride of V + 3; rows salted with NaN
    payloads, -0, infinities and subnormals; the Buffer form in place and the array form; more than one workgroup span per row."""
    rng = np.random.default_rng(V)
    sets = row_sets(rng, V)
    lb = wrk.LogitBias(ctx, V, sets)
    assert lb.num_sets == 4
    words = [NONE, 0, 1, 2, 3]
    for stride in (V, V + 3):
        a = TG.special_rows(rng, 5, stride)
        buf = ctx.buffer(a)
        assert ctx.bias_logits(buf, lb, words, num_vocab=V, row_stride=stride) is None
        got = buf.read(np.float32, a.size).reshape(5, stride)
        for r, w in enumerate(words):
            want = BR.apply(a[r, :V], *((None, None) if w == NONE else sets[w]))
            assert np.array_equal(bits(got[r, :V]), bits(want)), (stride, r)
            assert np.array_equal(bits(got[r, V:]), bits(a[r, V:])), "the padding between rows is not touched"
    dense = TG.special_rows(rng, 5, V)
    out = ctx.bias_logits(dense, lb, words)
    for r, w in enumerate(words):
        assert np.array_equal(bits(out[r]), bits(BR.apply(dense[r], *((None, None) if w == NONE else sets[w])))), r
    # the hand-worked cases of the contract: a ban on +inf, NaN and -inf, x + v on zeros and subnormals, an untouched -0
    if V >= 50:
        row = np.zeros((1, V), np.float32)
        row.view(np.uint32)[0, :11] = [0x7FC01234, 0xFFC00001, 0, 0x80000000, 0x7F800000, 0xFF800000, 0x3FC00000, 1, 0x807FFFFF, 0x00800000, 0x80000000]
        hand = wrk.LogitBias(ctx, V, [([0, 4, 5, 2, 3, 7, 8, 9, 6], [-INF, -INF, -INF, -0.0, 0.0, np.float32(1e-45), np.array([0x007FFFFF], np.uint32).view(np.float32)[0],
                                                                    -np.array([0x00800000], np.uint32).view(np.float32)[0], 1.0])])
        got = bits(ctx.bias_logits(row, hand, 0))[0, :11].tolist()
        assert got == [0xFF800000, 0xFFC00001, 0, 0, 0xFF800000, 0xFF800000, 0x40200000, 2, 0, 0, 0x80000000]
        hand.close()
    lb.close()


@pytest.mark.parametrize("V,in_stride,out_stride", [(512, 512, 512), (4100, 4100, 4104), (12288, 12288, 12288), (12288, 12292, 12288),
                                                     (4096, 4099, 4096), (4096, 4096, 4098), (4099, 4099, 4099), (1, 1, 5), (70001, 70004, 70001)])
def test_the_copying_launch_matches_the_restatement(ctx, V, in_stride, out_stride):
    """What a step program launches: rows of one buffer biased into the rows of another.  The decode loops reach it at V = 512 only (one
    workgroup span, 16-byte accesses), so it is run here through the library's test entry point: the 16-byte copy over several spans and
    with the last span cut short (V = 4100, 12288), and the scalar copy, taken when V % 4 != 0 or a stride is no multiple of 4.  The
    source rows and the padding of the destination stay as they were."""
    fn = wrk.hip.wrk_bias_rows_copy
    fn.restype, fn.argtypes = C.c_int32, [wrk._P, wrk._P, C.c_uint32, wrk._P, C.c_uint32, C.c_uint32, C.c_uint32, wrk._P, wrk._u32p]
    rng = np.random.default_rng(V + in_stride)
    sets = row_sets(rng, V)
    lb = wrk.LogitBias(ctx, V, sets)
    words = np.array([NONE, 0, 1, 2, 3], np.uint32)
    src = TG.special_rows(rng, 5, in_stride)
    canary = np.full((5, out_stride), 0x7FA5A5A5, np.uint32).view(np.float32)
    a, b = ctx.buffer(src), ctx.buffer(canary)
    ctx.check(fn(ctx.h, a.h, in_stride, b.h, out_stride, V, 5, lb.h, P_(words, wrk._u32p)))
    got = b.read(np.float32, canary.size).reshape(5, out_stride)
    assert np.array_equal(bits(a.read(np.float32, src.size)), bits(src).reshape(-1)), "the source rows are only read"
    for r, w in enumerate(words.tolist()):
        want = BR.apply(src[r, :V], *((None, None) if w == NONE else sets[w]))
        assert np.array_equal(bits(got[r, :V]), bits(want)), r
        assert np.array_equal(bits(got[r, V:]), bits(canary[r, V:])), "the padding between rows is not touched"
    assert fn(ctx.h, a.h, in_stride, a.h, in_stride, V, 5, lb.h, P_(words, wrk._u32p)) == wrk.E_ARG         # one buffer: wrk_bias_logits
    lb.close()


# ----------------------------------------------------------------------------- 2. validation
def test_create_argument_errors(ctx):
    V = 6

    def create(V=V, off=(0, 2, 2, 5), ids=(1, 4, 0, 5, 3), vals=(0.5, -np.inf, -3.0, -np.inf, 0.0), num_sets=None):
        o = None if off is None else np.array(off, np.uint32)
        i = None if ids is None else np.array(list(ids) + [0], np.uint32)
        v = None if vals is None else np.array(list(vals) + [0], np.float32)
        h = wrk._P()
        rc = wrk.hip.wrk_logit_bias_create(ctx.h, V, (len(off) - 1 if num_sets is None else num_sets) if off is not None else 1,
                                           None if o is None else P_(o, wrk._u32p), None if i is None else P_(i, wrk._u32p),
                                           None if v is None else P_(v, wrk._f32p), C.byref(h))
        if rc == wrk.OK:
            wrk.hip.wrk_logit_bias_destroy(h)
        else:
            assert not h.value
        want = BR.check_sets(V, off if num_sets is None or off is None else list(off)[:num_sets + 1], ids, vals)
        assert {"ok": wrk.OK, "arg": wrk.E_ARG, "unsupported": wrk.E_UNSUPPORTED}[want] == rc, (off, ids, vals)
        return rc

    assert create() == wrk.OK
    assert create(off=(0, 0), ids=(), vals=()) == wrk.OK                                            # one empty set
    assert create(off=None) == wrk.E_ARG and create(ids=None) == wrk.E_ARG and create(vals=None) == wrk.E_ARG   # NULL arrays
    assert create(off=(0,), num_sets=0) == wrk.E_ARG                                                # num_sets 0
    assert create(off=[0] * (wrk.MAX_BIAS_SETS + 1), ids=(), vals=()) == wrk.OK
    assert create(off=[0] * (wrk.MAX_BIAS_SETS + 2), ids=(), vals=()) == wrk.E_ARG                  # num_sets > WRK_MAX_BIAS_SETS
    assert create(off=(1, 2), ids=(0, 1), vals=(0.0, 0.0)) == wrk.E_ARG                             # offsets that do not start at 0
    assert create(off=(0, 2, 1), ids=(0, 1), vals=(0.0, 0.0)) == wrk.E_ARG                          # ... that decrease
    assert create(off=(0, 1), ids=(V,), vals=(0.0,)) == wrk.E_ARG                                   # an id >= num_vocab
    assert create(off=(0, 2), ids=(3, 3), vals=(0.0, 1.0)) == wrk.E_ARG                             # the same id twice in one set
    assert create(off=(0, 1, 2), ids=(3, 3), vals=(0.0, 1.0)) == wrk.OK                             # ... in two sets it is fine
    assert create(off=(0, 1), ids=(0,), vals=(np.nan,)) == wrk.E_ARG and create(off=(0, 1), ids=(0,), vals=(np.inf,)) == wrk.E_ARG
    assert create(off=(0, V), ids=range(V), vals=[-np.inf] * V) == wrk.E_ARG                        # a set that bans every token
    assert create(off=(0, V), ids=range(V), vals=[-np.inf] * (V - 1) + [-1e30]) == wrk.OK
    assert create(V=0) == wrk.E_ARG
    assert create(V=2 ** 20 + 1, off=(0, 0), ids=(), vals=()) == wrk.E_UNSUPPORTED
    with pytest.raises(ValueError):
        wrk.LogitBias(ctx, V, [([1, 2], [0.5])])


def test_argument_errors_leave_the_model_usable(ctx):
    V = vocab()
    rt = fresh(ctx, False, 2)
    lb = wrk.LogitBias(ctx, V, [{5: -np.inf}, {}, {7: 1.0}])
    other = wrk.LogitBias(ctx, V + 1, [{}])
    ctx2 = wrk.Context(0)
    foreign = wrk.LogitBias(ctx2, V, [{}])
    rt.generate_greedy([1, 2], 3)
    before = rt.state_back(0).copy()
    for kw in (dict(logit_bias=lb, bias_set=[0, 3]), dict(logit_bias=lb, bias_set=NONE - 1), dict(logit_bias=other), dict(logit_bias=foreign)):
        for call in (lambda: rt.generate_greedy([1, 2], 3, **kw), lambda: rt.generate_sample([1, 2], 3, **kw),
                     lambda: rt.generate_stop([1, 2], 3, [5], **kw), lambda: rt.generate_queue([[1, 2], [3]], max_new=2, **kw)):
            with pytest.raises(wrk.WrkError) as e:
                call()
            assert e.value.code == wrk.E_ARG, kw
    for bad in (lambda: ctx.bias_logits(np.zeros((1, V), np.float32), lb, [3]), lambda: ctx.bias_logits(np.zeros((1, V + 1), np.float32), lb, [0]),
                lambda: ctx.bias_logits(np.zeros((1, V), np.float32), foreign, [0])):
        with pytest.raises(wrk.WrkError) as e:
            bad()
        assert e.value.code == wrk.E_ARG
    with pytest.raises(ValueError):
        rt.generate_greedy([1, 2], 3, bias_set=[0, 0])
    # bias_set without bias, through the ABI
    ft, st = np.array([1, 2], np.uint32), np.zeros(2, np.uint32)
    out, lens, run = np.zeros((3, 2), np.uint32), np.zeros(2, np.uint32), C.c_uint32()
    opt = wrk.GenerateOptions()
    opt.bias_set = P_(st, wrk._u32p)
    assert wrk.hip.wrk_v7_generate_stop(ctx.h, rt.model, rt.state, P_(ft, wrk._u32p), 2, 3, C.byref(opt), P_(out, wrk._u32p), P_(lens, wrk._u32p),
                                        None, C.byref(run), None, 1) == wrk.E_ARG
    q = wrk.QueueOptions()
    pt, po, mn = np.array([1, 2, 3], np.uint32), np.array([0, 2, 3], np.uint32), np.array([2, 2], np.uint32)
    q.num_requests, q.prompt_tokens, q.prompt_offsets, q.max_new, q.max_steps = 2, P_(pt, wrk._u32p), P_(po, wrk._u32p), P_(mn, wrk._u32p), 8
    q.bias_set = P_(st, wrk._u32p)
    arrs = [np.zeros(4, np.uint32) for _ in range(5)]
    res = wrk.QueueResult(*[P_(a, wrk._u32p) for a in arrs], C.pointer(run))
    assert wrk.hip.wrk_v7_generate_queue(ctx.h, rt.model, rt.state, 2, C.byref(q), C.byref(res), None, 1) == wrk.E_ARG
    assert np.array_equal(bits(rt.state_back(0)), bits(before)), "a refused call launched nothing"
    # still usable: the greedy loop from a zero state equals a fresh runtime's, and a biased call runs
    zero_states(rt, 2)
    t, _ = rt.generate_greedy([1, 2], 4)
    fresh_rt = fresh(ctx, False, 2)
    assert np.array_equal(t, fresh_rt.generate_greedy([1, 2], 4)[0])
    fresh_rt.close()
    t, _ = rt.generate_greedy([1, 2], 4, logit_bias=lb, bias_set=[2, NONE])
    assert t.shape == (4, 2)
    rt.close()
    foreign.close()
    ctx2.close()
    other.close()
    lb.close()


# ----------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_an_empty_set_and_none_change_nothing(ctx, v6, mode, B, groups):
    V = vocab(v6)
    lb = wrk.LogitBias(ctx, V, [{3: -np.inf, 9: 2.0}, {}])
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    for family in FAMILIES:
        plain = run_loop(ctx, rt, family, B, mode, groups, occ=occ, logprobs=2)
        for word in (1, NONE):
            same(plain, run_loop(ctx, rt, family, B, mode, groups, occ=occ, logprobs=2, logit_bias=lb, bias_set=word), (family, word))
        # with stop sets: sequence 0 ends on its fourth token
        stops = [[int(plain["tok"][3, 0])]] + [[] for _ in range(B - 1)]
        plain = run_loop(ctx, rt, family, B, mode, groups, stop=stops, occ=occ, logprobs=2)
        assert plain["lens"][0] <= 4
        for word in (1, NONE):
            same(plain, run_loop(ctx, rt, family, B, mode, groups, stop=stops, occ=occ, logprobs=2, logit_bias=lb, bias_set=[word] * B),
                 (family, word, "with stops"))
    occ.close()
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 4. forced token
FORCED = [500, 3, 250, 77]


@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_a_huge_bias_forces_its_token(ctx, v6, mode, B, groups):
    V = vocab(v6)
    lb = wrk.LogitBias(ctx, V, [{t: 1e30} for t in FORCED])
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    want = np.tile(np.array(FORCED[:B], np.uint32), (STEPS, 1))
    for family in ("greedy", "sample", "filter", "pen"):
        out = run_loop(ctx, rt, family, B, mode, groups, occ=occ, logit_bias=lb, bias_set=list(range(B)))
        assert np.array_equal(out["tok"], want), family
    # the sets are per sequence: the same object, the words reversed
    out = run_loop(ctx, rt, "greedy", B, mode, groups, logit_bias=lb, bias_set=list(range(B))[::-1])
    assert np.array_equal(out["tok"], want[:, ::-1])
    occ.close()
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 5. bans against the occurrence table's
@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_bias_bans_equal_occurrence_bans(ctx, v6, mode, B, groups):
    V = vocab(v6)
    rng = np.random.default_rng(5)
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    kw = TG.cut(FAMILIES["sample"], B)

    def call(bans=None, **extra):
        zero_states(rt, B)
        for b in range(B):
            occ.load(b)
            if bans:
                occ.ban(b, bans[b])
        return rt.generate_penalized(FIRST[:B], STEPS, occ, presence=0.0, frequency=0.0, decay=1.0, mode=mode, groups=groups, **kw, **extra)[0]

    free = call()
    # every sequence bans what it drew without bans, and 100 random tokens: the banned call must go another way
    T = [sorted(set(free[:, b].tolist()) | set(rng.choice(V, 100, replace=False).tolist())) for b in range(B)]
    banned = call(bans=T)
    assert all(not (set(banned[:, b].tolist()) & set(T[b])) for b in range(B))
    lb = wrk.LogitBias(ctx, V, [{t: -np.inf for t in T[b]} for b in range(B)])
    biased = call(logit_bias=lb, bias_set=list(range(B)))
    assert np.array_equal(biased, banned)
    occ.close()
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 6. bans against a one-state automaton
@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_bias_bans_equal_a_one_state_automaton(ctx, v6, mode, B, groups):
    V = vocab(v6)
    rng = np.random.default_rng(6)
    inside = rng.random(V) < 0.5
    g = wrk.Grammar(ctx, V, np.where(inside, 0, 1).astype(np.uint16), [[0, G.REJECT]])
    lb = wrk.LogitBias(ctx, V, [(np.flatnonzero(~inside), np.full(int((~inside).sum()), -INF))])
    rt = fresh(ctx, v6, B)
    for family in ("greedy", "sample"):
        a = run_loop(ctx, rt, family, B, mode, groups, grammar=g)
        b = run_loop(ctx, rt, family, B, mode, groups, logit_bias=lb)           # bias_set None: set 0 for everyone
        assert np.array_equal(a["tok"], b["tok"]), family
        assert inside[a["tok"]].all()
        assert not np.array_equal(a["tok"], run_loop(ctx, rt, family, B, mode, groups)["tok"]), "the constraint changes nothing: no case"
    rt.close()
    lb.close()
    g.close()


# ----------------------------------------------------------------------------- 7. replay
REPLAY_SEED = {False: 157, True: 47}


@functools.lru_cache(maxsize=None)
def replay_sets(v6):
    V = vocab(v6)
    rng = np.random.default_rng(REPLAY_SEED[v6])
    sets = []
    for n in (64, 1, 200, 17):
        ids = rng.choice(V, n, replace=False)
        vals = rng.uniform(-4, 4, n).astype(np.float32)
        vals[rng.random(n) < 0.25] = -INF
        sets.append((ids, vals))
    return sets


def replay(ctx, v6, B, mode, family, sets, out):
    """A second runtime is fed the device's own tokens; the reference pick of `family` on bias_ref.apply of its logits (penalised through
    penalty_ref for "pen") must give the device's token wherever the reference does not call the row ambiguous.  (checked, steps)"""
    V = vocab(v6)
    rt = fresh(ctx, v6, B)
    pk = TG.picks_of(family, B)
    pen = TG.cut(FAMILIES["pen"], B) if family == "pen" else None
    counts = [np.zeros(V, np.float32) for _ in range(B)]
    flags = [np.zeros(V, np.uint32) for _ in range(B)]
    ones = np.ones(V, np.float32)
    cur = FIRST[:B]
    checked = total = 0
    for step in range(out["tok"].shape[0]):
        logits = rt.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
        for b in range(B):
            y = int(out["tok"][step, b])
            x = BR.apply(logits[b], *sets[b])
            assert x[y] != -np.inf, f"step {step} sequence {b}: token {y} is banned"
            if pen:
                x = R.penalize(x, counts[b], flags[b], pen["presence"][b], pen["frequency"][b])
                counts[b], flags[b] = R.update(counts[b], flags[b], y, ones, pen["decay"][b])
            tok, ambiguous = pk[b].draw(x, step)
            total += 1
            if not ambiguous:
                assert y == tok, (family, step, b)
                checked += 1
        cur = out["tok"][step].tolist()
    rt.close()
    return checked, total


@pytest.mark.parametrize("v6,mode,B,groups", CONFIGS)
def test_random_sets_match_the_replay(ctx, v6, mode, B, groups):
    V = vocab(v6)
    sets = replay_sets(v6)
    lb = wrk.LogitBias(ctx, V, sets)
    rt = fresh(ctx, v6, B)
    occ = wrk.Occurrence(ctx, B, V)
    checked = total = 0
    for family in FAMILIES:
        out = run_loop(ctx, rt, family, B, mode, groups, occ=occ, logit_bias=lb, bias_set=list(range(B)))
        c, t = replay(ctx, v6, B, mode, family, sets, out)
        print(f"{family}: {c} of {t} steps checked")
        checked, total = checked + c, total + t
        if family == "greedy":
            assert c == t, "greedy has no excused step"
            changed = int((out["tok"] != run_loop(ctx, rt, family, B, mode, groups)["tok"]).sum())
            print(f"the bias changes {changed} of {t} greedy picks")
            assert changed > 0, "the bias changes no greedy pick: a kernel that does nothing would pass"
        # with a stop set on sequence 0: a prefix of the tokens without it
        stops = [[int(out["tok"][4, 0])]] + [[] for _ in range(B - 1)]
        cut_ = run_loop(ctx, rt, family, B, mode, groups, occ=occ, stop=stops, logit_bias=lb, bias_set=list(range(B)), poll_steps=2)
        assert cut_["lens"][0] <= 5
        for b in range(B):
            n = int(cut_["lens"][b])
            assert cut_["tok"][:n, b].tolist() == out["tok"][:n, b].tolist(), (family, b)
    assert B != 4 or checked >= 0.95 * total, (checked, total)
    occ.close()
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 8. log-probs stay raw
@pytest.mark.parametrize("v6,mode,B", [(False, 1, 1), (False, 1, 4), (True, 1, 4), (False, 0, 4)])
def test_logprobs_stay_on_the_raw_head_output(ctx, v6, mode, B):
    V = vocab(v6)
    rt = fresh(ctx, v6, B)
    plain = run_loop(ctx, rt, "greedy", B, mode, 1)
    # every sequence bans its own unbiased first pick, the raw arg-max of step 0, and a few more tokens
    sets = [{11: -np.inf, 12: 3.0, 400: -2.0, int(plain["tok"][0, b]): -np.inf} for b in range(B)]
    lb = wrk.LogitBias(ctx, V, sets)
    words = list(range(B))
    out = run_loop(ctx, rt, "greedy", B, mode, 1, logit_bias=lb, bias_set=words, logprobs=5)
    lp, ids, tlp = out["lp"]
    for b in range(B):
        assert int(ids[0, b, 0]) == int(plain["tok"][0, b]) != int(out["tok"][0, b]), "the banned raw arg-max is alternative 0"
    for step in range(STEPS):
        # the head output the step's tokens were picked from: last_logits of the same call cut after that step
        head = run_loop(ctx, rt, "greedy", B, mode, 1, steps=step + 1, logit_bias=lb, bias_set=words)
        assert np.array_equal(head["tok"], out["tok"][:step + 1])
        want = ctx.top_logprobs(head["logits"], out["tok"][step], 5)
        assert np.array_equal(bits(lp[step]), bits(want[0])) and np.array_equal(ids[step], want[1]) and np.array_equal(bits(tlp[step]), bits(want[2])), step
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 9. the queue
QUEUE_PROMPTS = [3, 1, 4, 2, 1, 2]
QUEUE_NEW = [4, 6, 3, 5, 2, 6]
QUEUE_WORDS = [0, 1, NONE, 2, 1, 3]        # one request without a set, two sharing set 1


def queue_sets(V):
    rng = np.random.default_rng(9)
    sets = []
    for n in (150, 300, 40, 220):
        vals = rng.uniform(-6, 6, n).astype(np.float32)
        vals[rng.random(n) < 0.5] = -INF
        sets.append((rng.choice(V, n, replace=False), vals))
    return sets


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("v6,mode,B", [(False, 1, 1), (False, 1, 2), (False, 0, 3), (True, 1, 2)])
@pytest.mark.parametrize("family", ["greedy", "sample"])
def test_queue_requests_carry_their_own_set(ctx, family, v6, mode, B, pool):
    V = vocab(v6)
    n = len(QUEUE_PROMPTS)
    lb = wrk.LogitBias(ctx, V, queue_sets(V))
    prompts = [[(7 + 13 * r + 29 * i) % V for i in range(k)] for r, k in enumerate(QUEUE_PROMPTS)]
    kw = {k: np.resize(v, n) for k, v in FAMILIES[family].items()}
    rt = fresh(ctx, v6, B)
    sp = wrk.StatePool(ctx, rt, n) if pool else None

    def serve(order):
        pk = dict(pool=sp, save_state=list(range(len(order)))) if pool else {}
        got, _ = rt.generate_queue([prompts[r] for r in order], max_new=[QUEUE_NEW[r] for r in order], mode=mode, poll_steps=4, logit_bias=lb,
                                   bias_set=[QUEUE_WORDS[r] for r in order], **{k: v[order] for k, v in kw.items()}, **pk)
        return {r: got[i][0].tolist() for i, r in enumerate(order)}, got

    together, got = serve(list(range(n)))
    assert len({x[2] for x in got}) == B and all(x[1] == 2 for x in got)
    alone = {}
    for r in range(n):
        alone.update(serve([r])[0])
    assert together == alone, "a reply depends on the slot or the step its request was scheduled at"
    assert serve(list(range(n))[::-1])[0] == together
    # the sets matter: without them at least one reply is another
    free, _ = rt.generate_queue(prompts, max_new=QUEUE_NEW, mode=mode, **kw)
    assert [x[0].tolist() for x in free] != [together[r] for r in range(n)]
    assert free[2][0].tolist() == together[2], "the request with WRK_BIAS_NONE is served as without a bias"
    if sp:
        sp.close()
    rt.close()
    lb.close()


# ----------------------------------------------------------------------------- 10. programs
def test_one_program_serves_any_bias_and_any_sets(ctx):
    """The object and the set words are device data: a second object and other words replay the program the first call captured (the call
    would otherwise still follow the first object), and calls without a bias are unaffected in between."""
    V = vocab()
    rt = fresh(ctx, False, 2)
    plain, _ = rt.generate_greedy(FIRST[:2], 6)
    lb1 = wrk.LogitBias(ctx, V, [{t: 1e30} for t in FORCED])
    lb2 = wrk.LogitBias(ctx, V, [{9: 1e30}, {}, {8: 1e30, 9: -np.inf}])
    for _ in range(2):
        zero_states(rt, 2)
        a, _ = rt.generate_greedy(FIRST[:2], 6, logit_bias=lb1, bias_set=[0, 1])
        assert a.T.tolist() == [[FORCED[0]] * 6, [FORCED[1]] * 6]
        zero_states(rt, 2)
        a, _ = rt.generate_greedy(FIRST[:2], 6, logit_bias=lb1, bias_set=[3, 2])
        assert a.T.tolist() == [[FORCED[3]] * 6, [FORCED[2]] * 6]
        zero_states(rt, 2)
        b, _ = rt.generate_greedy(FIRST[:2], 6, logit_bias=lb2, bias_set=[0, 2])
        assert b.T.tolist() == [[9] * 6, [8] * 6]
        zero_states(rt, 2)
        c, _ = rt.generate_greedy(FIRST[:2], 6, logit_bias=lb2, bias_set=[1, NONE])
        assert np.array_equal(c, plain)
        zero_states(rt, 2)
        assert np.array_equal(rt.generate_greedy(FIRST[:2], 6)[0], plain)
    rt.close()
    lb1.close()
    lb2.close()
