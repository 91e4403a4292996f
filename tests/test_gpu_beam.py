"""Beam search on the device (web-rwkv-gguf_amd/csrc/wrk_beam.hip, wrk_beam_select.h) against tests/beam_ref.py, the rule in
NumPy written from the contract of wrk_v7_generate_beam in include/wrk_hip.h.  All comparisons are exact: ids, slots, bit patterns.
The loops run on the tiny fixtures (V = 512, D = 256, L = 2), RWKV-7 and RWKV-6, modes 0 and 1.

  1. state_permute   against state_back on the host: identity, a swap, a broadcast, a chain, many-to-one with fixed points, n < num_batch;
                     states of distinct per-slot bit patterns with NaN payloads and -0
  2. beam_step       against beam_ref on the log-probs Context.top_logprobs gives for the same rows: V in {1, 3, 512, 4097, 65536}, tight
                     rows and stride V + 3, W in {1, 2, 4, 16}, G in {1, 3}; rows with NaN, +-inf and equal logits; records that mix LIVE,
                     DONE and DEAD slots; rows with fewer than W finite logits
  3. identity        generate_beam(W = 1) returns generate_greedy's tokens, and its score is the sequential f32 sum of that call's
                     log-probs, bit for bit
  4. replay          a second runtime of the same B and mode is fed the device's own step tokens, its states permuted by the device's own
                     step parents through state_back / state_load; every step's selection is beam_ref on Context.top_logprobs of that
                     runtime's logits: tokens, parents, score bits per step, statuses and ranks at the end
  5. end states      every returned hypothesis's slot holds the state the replay has for it (a DONE slot: at the step that ended it), and
                     greedy decoding continues from it as from the replay's
  6. bias            banning the best hypothesis's first token changes rank 0 and no hypothesis contains it; BIAS_NONE is the identity
  7. every WRK_E_ARG of the contract
  8. generate_greedy / generate_stop return the same before and after a beam call on the same runtime

The replay is exact: on the MI355X the two runtimes' logits were bit-identical in every configuration (both models, modes 0 and 1), so no
group-step is excused and no tolerance exists.  The shape is the one worked out on the CPU for RWKV-7 with the oracle's logits (first
tokens 7, 100, 300, 411; 12 steps): at least 9 of 12 (W = 2) and 24 of 24 (W = 4) group-steps reorder slots, and the stop set
range(0, 512, 5) ends 8 of 8 beams within 12 steps at W = 4, G = 2, length_penalty 1.  Those counts were not re-derived on the CPU for
RWKV-6; instead test_replay asserts, for either model and every configuration, what they are there to guarantee: without stops at
least half of the group-steps have a non-empty copy list (a permutation that does nothing fails), and with the stop set at least one
hypothesis ends (the snapshot and the restore run).  Both held on the MI355X for all 16 parametrisations."""
import ctypes as C
import functools

import numpy as np
import pytest

import beam_ref as br
import wrk
from oracle import synth
from oracle.rnn import stack_cursors
from test_gpu_grammar import special_rows

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
NO = br.NO_TOKEN
FIRST = [7, 100, 300, 411]
STEPS = 12
STOPS = list(range(0, 512, 5))


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)


@pytest.fixture(scope="module")
def runtimes(ctx):
    """runtimes by (v6, num_batch, which): built once, states zeroed by the tests that need it"""
    made = {}

    def get(v6, B, which=0):
        if (v6, B, which) not in made:
            made[(v6, B, which)] = wrk.Runtime(ctx, wrk.GgufReader(model(v6)), num_batch=B)
        return made[(v6, B, which)]
    yield get
    for rt in made.values():
        rt.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def zero_states(rt, B):
    z = np.zeros_like(rt.state_back(0))
    for b in range(B):
        rt.state_load(z, b)


# ----------------------------------------------------------------------------- 1. state_permute
def patterned_state(rng, shape, b):
    """distinct per slot: random words with the slot number in the low byte, NaN payloads, infinities and -0 sprinkled in"""
    u = (rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFFFFFF00)) | np.uint32(b)
    where = rng.random(shape)
    u[where < 0.05] = np.uint32(0x7FC01200 | b)
    u[(where >= 0.05) & (where < 0.1)] = np.uint32(0x80000000)
    u[(where >= 0.1) & (where < 0.12)] = np.uint32(0xFFC00100 | b)
    return u.view(np.float32)


MAPS = {4: [[0, 1, 2, 3], [1, 0, 3, 2], [0, 0, 0, 0], [1, 2, 3, 0], [3, 3, 1, 1], [1, 1, 0]],
        8: [[0, 1, 2, 3, 4, 5, 6, 7], [1, 0, 3, 2], [0, 0, 0, 0], [1, 2, 3, 0], [3, 3, 1, 1, 4, 5, 5, 0], [1, 2, 3, 4, 5, 6, 7, 0], [4, 4, 4, 0, 1]]}


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("num_batch", [4, 8])
def test_state_permute(ctx, runtimes, v6, num_batch):
    rt = runtimes(v6, num_batch)
    rng = np.random.default_rng(5 + num_batch)
    shape = rt.state_back(0).shape
    for m in MAPS[num_batch]:
        before = [patterned_state(rng, shape, b) for b in range(num_batch)]
        for b in range(num_batch):
            rt.state_load(before[b], b)
        rt.state_permute(m)
        for q in range(num_batch):
            want = before[m[q]] if q < len(m) else before[q]            # slots >= n untouched
            assert np.array_equal(bits(rt.state_back(q)), bits(want)), (m, q)
    with pytest.raises(wrk.WrkError) as e:
        rt.state_permute([0] * (num_batch + 1))                         # more slots than the state has
    assert e.value.code == wrk.E_ARG
    with pytest.raises(wrk.WrkError) as e:
        rt.state_permute([0, 2])                                        # a parent outside [0, n)
    assert e.value.code == wrk.E_ARG


# ----------------------------------------------------------------------------- 2. beam_step
def step_rows(rng, B, V, stride):
    """rows of three kinds: special_rows (NaN, +-inf, -0, equal values), finite rows with ties and -inf, rows with few finite logits"""
    a = special_rows(rng, B, stride)
    for b in range(B):
        kind = b % 3
        if kind == 1:
            a[b] = rng.integers(-6, 3, stride).astype(np.float32) * np.float32(0.5)        # many equal logits
            a[b, rng.random(stride) < 0.2] = -np.inf
        elif kind == 2:
            a[b] = -np.inf
            keep = rng.choice(V, min(V, int(rng.integers(1, 4))), replace=False)          # 1 to 3 finite logits: fewer than W for W >= 4
            a[b, keep] = rng.normal(0, 2, keep.size).astype(np.float32)
    return a


def random_records(rng, B, alpha, inv):
    length = rng.integers(0, 6, B).astype(np.uint32)
    status = rng.choice([br.DEAD, br.LIVE, br.LIVE, br.LIVE, br.DONE], B).astype(np.uint32)
    score = (-rng.integers(0, 40, B) * 0.25).astype(np.float32)
    key = np.array([np.float32(score[b] * inv[max(int(length[b]), 1)]) for b in range(B)], np.float32)
    score[status == br.DEAD] = -np.inf
    key[status == br.DEAD] = -np.inf
    return score, key, length, status


@pytest.mark.parametrize("V", [1, 3, 512, 4097, 65536])
@pytest.mark.parametrize("W", [1, 2, 4, 16])
def test_beam_step_matches_the_reference(ctx, V, W):
    rng = np.random.default_rng(1000 * W + V % 997)
    for G in (1, 3):
        for stride in (V, V + 3):
            for alpha in (0.0, 1.0):
                B = G * W
                rows = step_rows(rng, B, V, stride)
                buf = ctx.buffer(rows)
                inv = br.inv_norm_table(alpha, 8)
                score, key, length, status = random_records(rng, B, alpha, inv)
                if alpha == 0.0 and stride == V:
                    score, key, length, status = br.start_records(G, W)                    # the start of a call
                stops = [[int(x) for x in rng.choice(V, min(V, 5), replace=False)] for _ in range(G)]
                _, ids, lp = ctx.top_logprobs(buf, np.zeros(B, np.uint32), W, num_vocab=V, row_stride=stride)
                want = br.select(score, key, length, status, ids, lp, W, inv, stops)
                tok, par, cp, s2, k2, l2, st2 = ctx.beam_step(buf, W, score, key, length, status, stop=stops, length_penalty=alpha, num_vocab=V,
                                                              row_stride=stride)
                what = (V, W, G, stride, alpha)
                assert np.array_equal(tok, want["token"]) and np.array_equal(par, want["parent"]), what
                assert np.array_equal(cp, want["copy_src"]), what
                assert np.array_equal(bits(s2), bits(want["score"])) and np.array_equal(bits(k2), bits(want["key"])), what
                assert np.array_equal(l2, want["length"]) and np.array_equal(st2, want["status"]), what


# ----------------------------------------------------------------------------- 3. W = 1 is greedy with a score
@pytest.mark.parametrize("v6,mode,G", [(False, 0, 1), (False, 1, 1), (False, 1, 4), (True, 0, 1), (True, 1, 4)])
def test_one_beam_is_greedy(ctx, runtimes, v6, mode, G):
    rt = runtimes(v6, G)
    zero_states(rt, G)
    tok, _ = rt.generate_greedy(FIRST[:G], STEPS, mode=mode, logprobs=0)
    lp = rt.last_logprobs[0]
    zero_states(rt, G)
    res, run = rt.generate_beam(FIRST[:G], STEPS, 1, mode=mode)
    assert run == STEPS
    for g in range(G):
        (toks, score, finished, slot), = res[g]
        assert toks.tolist() == tok[:, g].tolist() and not finished and slot == g
        acc = np.float32(0.0)
        for s in range(STEPS):
            acc = np.float32(acc + lp[s, g])
        assert bits(np.float32(score)) == bits(acc), (g, score, acc)


# ----------------------------------------------------------------------------- 4 and 5. replay and end states
def replay(ctx, rt, rt2, v6, mode, W, G, alpha, stop):
    B = G * W
    first = FIRST[:G]
    zero_states(rt, B)
    zero_states(rt2, B)
    res, run = rt.generate_beam(first, STEPS, W, stop=stop, length_penalty=alpha, mode=mode)
    d_tok, d_par, d_score = rt.last_beam_steps
    assert d_tok.shape == (run, B)
    inv = br.inv_norm_table(alpha, STEPS)
    stops = [list(stop or [])] * G
    score, key, length, status = br.start_records(G, W)
    cur = np.repeat(np.asarray(first, np.uint32), W)
    frozen = {}                     # slot -> the replay's state at the step that ended it
    moved = ended = 0
    for s in range(run):
        logits = rt2.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
        _, ids, lp = ctx.top_logprobs(logits, np.zeros(B, np.uint32), W)
        want = br.select(score, key, length, status, ids, lp, W, inv, stops)
        what = (v6, mode, W, G, alpha, bool(stop), s)
        assert np.array_equal(d_tok[s], want["token"]), what
        assert np.array_equal(d_par[s], want["parent"]), what
        assert np.array_equal(bits(d_score[s]), bits(want["score"])), what
        # the replay's states move as the device's own parents say
        states = {int(p): rt2.state_back(int(p)) for p in set(d_par[s][d_tok[s] != NO].tolist())}
        for q in range(B):
            if d_tok[s][q] != NO and d_par[s][q] != q:
                rt2.state_load(states[int(d_par[s][q])], q)
            if d_tok[s][q] != NO:
                cur[q] = d_tok[s][q]
            if want["ended"][q]:
                frozen[q] = rt2.state_back(q)
            elif want["status"][q] != br.DONE:
                frozen.pop(q, None)
        for g in range(G):
            moved += int((want["copy_src"][g * W:(g + 1) * W] != br.NO_COPY).any())
        ended += int(want["ended"].sum())
        score, key, length, status = want["score"], want["key"], want["length"], want["status"]
    assert run == STEPS or not (status == br.LIVE).any()
    # the hypotheses: ranks, tokens, scores, flags and slots
    order = br.hypotheses(key, status, W)
    for g in range(G):
        assert [h[3] for h in res[g]] == order[g], (v6, mode, W, G, alpha, g)
        for toks, sc, fin, slot in res[g]:
            assert toks.tolist() == br.backtrack(d_tok, d_par, slot, int(length[slot]))
            assert bits(np.float32(sc)) == bits(score[slot]) and fin == (status[slot] == br.DONE)
            # 5. the slot holds the state that has consumed everything but the last token
            want_state = frozen[slot] if fin else rt2.state_back(slot)
            assert np.array_equal(bits(rt.state_back(slot)), bits(want_state)), (v6, mode, W, G, alpha, slot, fin)
    return res, run, moved, frozen, ended


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,G", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_replay(ctx, runtimes, v6, mode, W, G):
    rt, rt2 = runtimes(v6, W * G, 0), runtimes(v6, W * G, 1)
    for alpha in (0.0, 1.0):
        for stop in (None, STOPS):
            res, run, moved, frozen, done = replay(ctx, rt, rt2, v6, mode, W, G, alpha, stop)
            if stop is None:
                assert run == STEPS and done == 0
                # a permutation that does nothing cannot pass: at least half of the group-steps move a slot
                assert moved >= (run * G) // 2, (moved, run, G)
            else:
                assert done >= 1, "the stop set ends no beam: the snapshot path is not exercised"
    # 5, the second half: greedy decoding from the slots continues as from the replay's states (the last configuration's)
    B = W * G
    last = np.zeros(B, np.uint32)
    for g in range(G):
        for toks, _, fin, slot in res[g]:
            last[slot] = toks[-1]
            if fin:
                rt2.state_load(frozen[slot], slot)
    a, _ = rt.generate_greedy(last, 4, mode=mode)
    b, _ = rt2.generate_greedy(last, 4, mode=mode)
    live = [slot for g in range(G) for _, _, _, slot in res[g]]
    assert np.array_equal(a[:, live], b[:, live])


# ----------------------------------------------------------------------------- 6. bias
@pytest.mark.parametrize("v6", [False, True])
def test_bias_bans_and_identity(ctx, runtimes, v6):
    W, G, V = 4, 1, 512
    rt = runtimes(v6, W * G)

    def run(**kw):
        zero_states(rt, W * G)
        res, _ = rt.generate_beam(FIRST[:G], 8, W, mode=1, **kw)
        return [[(t.tolist(), bits(np.float32(s)).tolist(), f, q) for t, s, f, q in grp] for grp in res]
    plain = run()
    t0 = plain[0][0][0][0]
    lb = wrk.LogitBias(ctx, V, [{t0: -np.inf}])
    banned = run(logit_bias=lb)
    assert banned[0][0][0] != plain[0][0][0]
    assert all(t0 not in toks for toks, _, _, _ in banned[0])
    assert run(logit_bias=lb, bias_set=wrk.BIAS_NONE) == plain
    lb.close()


# ----------------------------------------------------------------------------- 7. validation
def raw_beam(rt, first, steps, W, gen=None, alpha=0.0, mode=1, drop=None, G=None):
    """wrk_v*_generate_beam below Runtime.generate_beam: the status code"""
    ft = np.asarray(first, np.uint32)
    G = ft.size if G is None else G
    n = max(G * max(W, 1), 1)
    arr = dict(tokens=np.zeros(n * max(steps, 1), np.uint32), lengths=np.zeros(n, np.uint32), scores=np.zeros(n, np.float32),
               finished=np.zeros(n, np.uint32), slots=np.zeros(n, np.uint32), num_hyps=np.zeros(max(G, 1), np.uint32), steps_run=np.zeros(1, np.uint32))
    res = wrk.BeamResult(**{k: P_(v, wrk._f32p if v.dtype == np.float32 else wrk._u32p) for k, v in arr.items() if k != drop})
    opt = wrk.BeamOptions(W, alpha, C.pointer(gen) if gen is not None else None)
    fn, mdl = rt._entry("generate_beam")
    ms = C.c_float()
    return fn(rt.ctx.h, mdl, rt.state, P_(ft, wrk._u32p), G, steps, C.byref(opt), C.byref(res), C.byref(ms), mode)


@pytest.mark.parametrize("v6", [False, True])
def test_argument_errors(ctx, runtimes, v6):
    rt = runtimes(v6, 4)
    V = 512
    ok = raw_beam(rt, [7], 2, 2)
    assert ok == wrk.OK
    bad = []
    bad.append(raw_beam(rt, [7], 2, 0))                                 # W out of range
    bad.append(raw_beam(rt, [7], 2, 17))
    bad.append(raw_beam(rt, [7, 8, 9], 2, 2))                           # G * W above the state's batch
    bad.append(raw_beam(rt, [7], 2, 8))
    for a in (-0.5, float("inf"), float("nan"), 1000.0):                # length_penalty; 1000: 1 / 2^1000 is no normal f32
        bad.append(raw_beam(rt, [7], 2, 2, alpha=a))
    bad.append(raw_beam(rt, [V], 2, 2))                                 # a first token >= num_vocab
    bad.append(raw_beam(rt, [7], 0, 2))                                 # steps == 0
    bad.append(raw_beam(rt, [7], 2, 2, mode=1 | (2 << 8)))              # lanes
    bad.append(raw_beam(rt, [7], 2, 2, drop="lengths"))                 # a NULL required array
    keep = []

    def gen(**kw):
        g = wrk.GenerateOptions()
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = P_(v, wrk._f32p if v.dtype == np.float32 else wrk._u32p)
            setattr(g, k, v)
        return g
    one_f, one_u = np.ones(4, np.float32), np.ones(4, np.uint32)
    bad.append(raw_beam(rt, [7], 2, 2, gen(stop_tokens=np.array([V], np.uint32), stop_offsets=np.array([0, 1], np.uint32))))   # stop id >= vocab
    bad.append(raw_beam(rt, [7], 2, 2, gen(stop_tokens=np.zeros(129, np.uint32), stop_offsets=np.array([0, 129], np.uint32))))   # too many stop ids
    bad.append(raw_beam(rt, [7], 2, 2, gen(stop_offsets=np.array([1, 1], np.uint32))))                                          # offsets not from 0
    bad.append(raw_beam(rt, [7], 2, 2, gen(bias_set=one_u)))                                                                    # bias_set without bias
    bad.append(raw_beam(rt, [7], 2, 2, gen(temperature=one_f, top_p=one_f, seed=one_u)))                                        # a sampler
    bad.append(raw_beam(rt, [7], 2, 2, gen(top_k=one_u)))
    bad.append(raw_beam(rt, [7], 2, 2, gen(typical_p=one_f)))
    bad.append(raw_beam(rt, [7], 2, 2, gen(mirostat_tau=one_f)))
    bad.append(raw_beam(rt, [7], 2, 2, gen(presence=one_f)))                                                                    # penalties
    bad.append(raw_beam(rt, [7], 2, 2, gen(no_repeat_ngram=one_u)))                                                             # DRY
    bad.append(raw_beam(rt, [7], 2, 2, gen(grammar_state=one_u)))                                                               # a grammar
    bad.append(raw_beam(rt, [7], 2, 2, gen(out_logprob=one_f)))                                                                 # log-probs
    bad.append(raw_beam(rt, [7], 2, 2, gen(num_top=1)))
    occ = wrk.Occurrence(ctx, 4, V)
    g = wrk.GenerateOptions()
    g.occ = occ.h
    bad.append(raw_beam(rt, [7], 2, 2, g))
    lb = wrk.LogitBias(ctx, V, [{1: 1.0}])
    g = wrk.GenerateOptions()
    g.bias = lb.h
    g.bias_set = P_(np.array([5], np.uint32), wrk._u32p)                # a set word that is neither < num_sets nor BIAS_NONE
    bad.append(raw_beam(rt, [7], 2, 2, g))
    assert bad == [wrk.E_ARG] * len(bad), bad
    lb.close()
    occ.close()
    # the row function
    rows = np.zeros((2, 8), np.float32)
    rec = br.start_records(1, 2)
    for kw in (dict(length_penalty=-1.0), dict(length_penalty=float("nan")), dict(stop=[9])):
        with pytest.raises(wrk.WrkError) as e:
            ctx.beam_step(rows, 2, *rec, **kw)
        assert e.value.code == wrk.E_ARG
    with pytest.raises(wrk.WrkError) as e:
        ctx.beam_step(rows, 2, rec[0], rec[1], rec[2], [3, 0])          # a status above DONE
    assert e.value.code == wrk.E_ARG
    with pytest.raises(wrk.WrkError) as e:
        ctx.beam_step(np.zeros((17, 8), np.float32), 17, *br.start_records(1, 17))
    assert e.value.code == wrk.E_ARG


# ----------------------------------------------------------------------------- 8. the other loops are undisturbed
@pytest.mark.parametrize("v6,mode", [(False, 0), (False, 1), (True, 1)])
def test_other_loops_are_undisturbed(ctx, runtimes, v6, mode):
    B = 4
    rt = runtimes(v6, B)

    def others():
        zero_states(rt, B)
        a, _ = rt.generate_greedy(FIRST, 8, mode=mode)
        zero_states(rt, B)
        b, lens = rt.generate_stop(FIRST, 8, STOPS[:wrk.MAX_STOP_TOKENS], mode=mode)
        return a.tolist(), b.tolist(), lens.tolist()
    before = others()
    zero_states(rt, B)
    rt.generate_beam(FIRST[:2], 8, 2, stop=STOPS, length_penalty=1.0, mode=mode)
    assert others() == before
