"""Beam search with a context per hypothesis on the device (wrk_v*_generate_beam_context, web-rwkv-gguf_amd/csrc/wrk_beam.hip, DESIGN.md
§7u) against tests/beam_ctx_ref.py.  All comparisons are exact: ids, slots, bit patterns.  The loops run on the tiny fixtures (V = 512,
D = 256, L = 2), RWKV-7 and RWKV-6, modes 0 and 1, with the vocabulary narrowed to the six tokens range(3, 512, 85) by a bias set, so
that hypotheses repeat themselves and the contexts bite (tests/test_beam_ctx_ref.py works the shape out on the CPU).

  1. permutations    occ.permute / win.permute against the host with test_gpu_beam's maps; rows of distinct per-slot patterns; V in
                     {1, 3, 512, 4097}, capacities {1, 5, 4096}, partly filled and wrapped rings; slots >= n untouched; both WRK_E_ARG
  2. replay          test_gpu_beam's method with a context: a second runtime is fed the device's tokens and permuted by the device's
                     parents, the host keeps every slot's context in NumPy (beam_ctx_ref) and loads it into replay-side tables, and every
                     step's selection is beam_ref on Context.top_logprobs of the replay's rows after bias_logits / penalize_logits /
                     dry_logits / constrain_logits.  Tokens, parents and score bits per step, statuses and ranks at the end
  3. identity        W = 1 with each context is the greedy call with the same context: tokens, occurrence row, window, automaton state;
                     an empty context is the plain beam call
  4. end contexts    every returned hypothesis's slot holds the replay's context for it, and a penalised greedy continuation from it
                     equals the replay's (inside the replay test)
  5. semantics       no hypothesis under no_repeat_ngram = n repeats an n-gram, the prompt given by win.add included, and the same call
                     without the ban does; Grammar.walk accepts every hypothesis of a grammar call; a ban set on slot gW alone holds for
                     every hypothesis of the group
  6. validation      every new WRK_E_ARG, and every refusal that remains on the new entry points
  7. undisturbed     generate_beam without context, generate_greedy, generate_stop and a penalised generate_stop return the same before
                     and after a context call on the same runtime"""
import ctypes as C
import functools

import numpy as np
import pytest

import beam_ctx_ref as bc
import beam_ref as br
import dry_ref
import grammar_ref
import penalty_ref
import wrk
from oracle import synth
from oracle.rnn import stack_cursors
from test_gpu_beam import MAPS, STEPS, bits, zero_states

pytestmark = pytest.mark.gpu

P_ = wrk._ptr
NO = br.NO_TOKEN
V = 512
ALLOWED = list(range(3, 512, 85))       # 3 88 173 258 343 428
FIRST = [3, 88]
STOPS = [428]
PROMPTS = [[88, 173], [3, 258, 3]]      # what slot gW's window and occurrence row hold before the call
CAPACITY = 64


@pytest.fixture(scope="module")
def ctx():
    c = wrk.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def model(v6=False):
    return synth.make_v6_gguf(synth.V6_CONFIGS["tiny"], 42) if v6 else synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)


@pytest.fixture(scope="module")
def made(ctx):
    """runtimes by (v6, num_batch, which), tables by (kind, num_batch, which), the six-token bias and the grammars: built once"""
    box = {}

    def get(kind, *key):
        k = (kind,) + key
        if k not in box:
            if kind == "rt":
                box[k] = wrk.Runtime(ctx, wrk.GgufReader(model(key[0])), num_batch=key[1])
            elif kind == "occ":
                box[k] = wrk.Occurrence(ctx, key[0], V)
            elif kind == "win":
                box[k] = wrk.TokenWindow(ctx, key[0], V, CAPACITY)
            elif kind == "bias":
                box[k] = wrk.LogitBias(ctx, V, [{t: -np.inf for t in range(V) if t not in ALLOWED}])
            elif kind == "choices":
                cls, trans, start = wrk.grammar_from_choices(V, [[88, 173, 88, 173, 3], [88, 3, 343], [173, 3, 3, 258], [3, 88, 88], [258, 343]], 428)
                box[k] = (wrk.Grammar(ctx, V, cls, trans), [start, start])
            elif kind == "dense":
                box[k] = (wrk.Grammar(ctx, V, *wrk.grammar_from_dense(dense_table())), [0, 3])
        return box[k]
    yield get
    for v in box.values():
        (v[0] if isinstance(v, tuple) else v).close()


def dense_table():
    """grammar_ref.random_dense over the vocabulary; among the six allowed tokens every state allows exactly two, so a beam has a way on
    and the mask still cuts its row"""
    S = 6
    t = grammar_ref.random_dense(np.random.default_rng(11), S, V, 48)
    for s in range(S):
        t[s, ALLOWED] = -1
        t[s, ALLOWED[s % 6]] = (s + 1) % S
        t[s, ALLOWED[(s + 2) % 6]] = (s + 4) % S
    return t


# ----------------------------------------------------------------------------- 1. the stand-alone permutations
@pytest.mark.parametrize("vocab", [1, 3, 512, 4097])
@pytest.mark.parametrize("num_batch", [4, 8])
def test_occurrence_permute(ctx, vocab, num_batch):
    occ = wrk.Occurrence(ctx, num_batch, vocab)
    rng = np.random.default_rng(vocab + num_batch)
    for m in MAPS[num_batch]:
        before = []
        for b in range(num_batch):
            counts = (rng.integers(0, 1 << 16, vocab) * 256 + b).astype(np.float32)      # exact in f32, the slot number in the low bits
            flags = rng.integers(0, 4, vocab).astype(np.uint32)
            flags[b % vocab] &= 1                                           # a slot may not ban its whole vocabulary
            occ.load(b, counts, flags)
            before.append((counts, flags))
        occ.permute(m)
        for q in range(num_batch):
            want = before[m[q]] if q < len(m) else before[q]            # slots >= n untouched
            c, f = occ.back(q)
            assert np.array_equal(bits(c), bits(want[0])) and np.array_equal(f, want[1]), (m, q)
    for bad in ([0] * (num_batch + 1), [0, 2]):                         # more slots than the table has; a parent outside [0, n)
        with pytest.raises(wrk.WrkError) as e:
            occ.permute(bad)
        assert e.value.code == wrk.E_ARG
    occ.close()


@pytest.mark.parametrize("capacity", [1, 5, 4096])
@pytest.mark.parametrize("num_batch", [4, 8])
def test_window_permute(ctx, capacity, num_batch):
    win = wrk.TokenWindow(ctx, num_batch, V, capacity)
    rng = np.random.default_rng(capacity + num_batch)
    for m in MAPS[num_batch]:
        before = []
        for b in range(num_batch):
            # empty, partly filled, exactly full, wrapped (more pushes than the ring holds), by slot
            n = [0, max(capacity // 2, 1), capacity, capacity + 3][b % 4]
            toks = ((rng.integers(0, V // 8, n) * 8 + b) % V).astype(np.uint32)
            win.load(b, None)
            if n:
                win.add(b, toks)
            before.append(toks[-capacity:] if n else toks)
        win.permute(m)
        for q in range(num_batch):
            want = before[m[q]] if q < len(m) else before[q]
            assert np.array_equal(win.back(q), want), (m, q)
        # the moved slot goes on as its source would: one more push
        win.add(0, [7])
        src = before[m[0]]
        assert np.array_equal(win.back(0), np.append(src, np.uint32(7))[-capacity:])
    for bad in ([0] * (num_batch + 1), [0, 2]):
        with pytest.raises(wrk.WrkError) as e:
            win.permute(bad)
        assert e.value.code == wrk.E_ARG
    win.close()


# ----------------------------------------------------------------------------- the contexts of the loop tests
CONTEXTS = ["ngram", "penalties", "dry", "choices", "dense", "all"]


def setup(made, name, G, W, which):
    """(keyword arguments of generate_beam, one beam_ctx_ref.group_params per group, the tables) of context `name` on G * W slots"""
    B = G * W
    occ = win = g = None
    kw, par = {}, [dict() for _ in range(G)]
    if name in ("penalties", "all"):
        occ = made("occ", B, which)
        pres, freq = [0.5, 0.25][:G], [0.5, 0.75][:G]
        kw.update(occurrence=occ, presence=pres, frequency=freq, decay=0.99)
        for k in range(G):
            par[k].update(presence=pres[k], frequency=freq[k], decay=0.99)
    if name in ("ngram", "dry", "all"):
        win = made("win", B, which)
        kw.update(window=win)
        nr = {"ngram": [2, 2], "dry": None, "all": [3, 2]}[name]
        dry = None if name == "ngram" else (0.75, 1.75, [1, 2][:G])
        if nr:
            kw.update(no_repeat_ngram=nr[:G])
        if dry:
            kw.update(dry=dry, dry_breakers=[343])
        for k in range(G):
            d = dict(no_repeat_ngram=nr[k] if nr else 0)
            if dry:
                d.update(multiplier=dry[0], base=dry[1], allowed_length=dry[2][k], breakers=(343,))
            par[k].update(capacity=CAPACITY, dry=d)
    if name in ("choices", "dense", "all"):
        g, starts = made("choices" if name == "choices" else "dense")
        kw.update(grammar=g, grammar_state=starts[:G])
        for k in range(G):
            par[k].update(grammar=(g.token_class, g.transitions))
    return kw, [bc.group_params(V, **p) for p in par], (occ, win, g)


def start_contexts(kw, pars, tables, G, W):
    """Puts the groups' prompts into slot gW of the tables and junk into the other slots; returns the host's B contexts"""
    occ, win, g = tables
    ctxs = []
    for q in range(G * W):
        k = q // W
        c = bc.new_context(V, kw["grammar_state"][k] if g else 0)
        toks = PROMPTS[k] if q % W == 0 else [428, 428, 343]
        if occ:
            occ.load(q)
            occ.add(q, toks, pars[k]["decay"])
            c["counts"], c["flags"] = penalty_ref.update_all(c["counts"], c["flags"], toks, pars[k]["weights"], pars[k]["decay"])
        if win:
            win.load(q, toks)
            c["window"] = list(toks)
        ctxs.append(c)
    return ctxs


def load_contexts(ctxs, occ, win):
    for q, c in enumerate(ctxs):
        if occ:
            occ.load(q, c["counts"], c["flags"])
        if win:
            win.load(q, c["window"])


def context_rows(ctx, rows, ctxs, kw, tables2, W):
    """the replay's rows after the stages of the chain, on tables that hold the host's contexts"""
    occ2, win2, g = tables2
    B = len(ctxs)
    per_slot = lambda v: np.repeat(np.asarray(v), W) if np.ndim(v) else v
    load_contexts(ctxs, occ2, win2)
    if occ2:
        rows = ctx.penalize_logits(rows, occ2, per_slot(kw["presence"]), per_slot(kw["frequency"]))
    if win2:
        dry = kw.get("dry")
        rows = ctx.dry_logits(rows, win2, dry=None if dry is None else tuple(per_slot(v) for v in dry),
                              no_repeat_ngram=None if kw.get("no_repeat_ngram") is None else per_slot(kw["no_repeat_ngram"]),
                              dry_breakers=kw.get("dry_breakers"))
    if g:
        rows = ctx.constrain_logits(rows, g, [c["state"] for c in ctxs])
    return rows


def check_contexts(rt, ctxs, tables, slots, what):
    occ, win, g = tables
    for q in slots:
        if occ:
            c, f = occ.back(q)
            assert np.array_equal(bits(c), bits(ctxs[q]["counts"])) and np.array_equal(f, ctxs[q]["flags"]), what + (q, "occurrence")
        if win:
            assert win.back(q).tolist() == ctxs[q]["window"], what + (q, "window")
        if g:
            assert int(rt.last_grammar_state[q]) == ctxs[q]["state"], what + (q, "state")


# ----------------------------------------------------------------------------- 2 and 4. replay and end contexts
def replay(ctx, made, v6, mode, W, G, alpha, stop, name):
    B = G * W
    rt, rt2 = made("rt", v6, B, 0), made("rt", v6, B, 1)
    lb = made("bias")
    kw, pars, tables = setup(made, name, G, W, 0)
    _, _, tables2 = setup(made, name, G, W, 1)
    first = FIRST[:G]
    zero_states(rt, B)
    zero_states(rt2, B)
    ctxs = start_contexts(kw, pars, tables, G, W)
    res, run = rt.generate_beam(first, STEPS, W, stop=stop, length_penalty=alpha, mode=mode, logit_bias=lb, **kw)
    d_tok, d_par, d_score = rt.last_beam_steps
    assert d_tok.shape == (run, B)
    inv = br.inv_norm_table(alpha, STEPS)
    stops = [list(stop or [])] * G
    score, key, length, status = br.start_records(G, W)
    cur = np.repeat(np.asarray(first, np.uint32), W)
    frozen = {}
    bitten = ended = moved = 0
    zeros = np.zeros(B, np.uint32)
    what = (v6, mode, W, G, alpha, bool(stop), name)
    for s in range(run):
        logits = rt2.infer_raw(cur, stack_cursors([1] * B), list(range(B)), mode=mode)
        biased = ctx.bias_logits(logits, lb, 0)
        rows = context_rows(ctx, biased, ctxs, kw, tables2, W)
        _, ids0, lp0 = ctx.top_logprobs(biased, zeros, W)
        _, ids, lp = ctx.top_logprobs(rows, zeros, W)
        live = status == br.LIVE
        bitten += int(((ids0 != ids).any(axis=1) | (bits(lp0) != bits(lp)).any(axis=1))[live].sum())
        want = br.select(score, key, length, status, ids, lp, W, inv, stops)
        assert np.array_equal(d_tok[s], want["token"]), what + (s,)
        assert np.array_equal(d_par[s], want["parent"]), what + (s,)
        assert np.array_equal(bits(d_score[s]), bits(want["score"])), what + (s,)
        # the replay's states and the host's contexts move as the device's own parents say, then the filled slots count their tokens
        states = {int(p): rt2.state_back(int(p)) for p in set(d_par[s][d_tok[s] != NO].tolist())}
        ctxs = bc.permute(ctxs, want["copy_src"])
        for q in range(B):
            if d_tok[s][q] != NO and d_par[s][q] != q:
                rt2.state_load(states[int(d_par[s][q])], q)
            if d_tok[s][q] != NO:
                cur[q] = d_tok[s][q]
                bc.count_token(ctxs[q], d_tok[s][q], pars[q // W])
            if want["ended"][q]:
                frozen[q] = rt2.state_back(q)
            elif want["status"][q] != br.DONE:
                frozen.pop(q, None)
        ended += int(want["ended"].sum())
        moved += int((want["copy_src"] != br.NO_COPY).sum())
        score, key, length, status = want["score"], want["key"], want["length"], want["status"]
    assert run == STEPS or not (status == br.LIVE).any()
    order = br.hypotheses(key, status, W)
    for g in range(G):
        assert [h[3] for h in res[g]] == order[g], what + (g,)
        for toks, sc, fin, slot in res[g]:
            assert toks.tolist() == br.backtrack(d_tok, d_par, slot, int(length[slot]))
            assert bits(np.float32(sc)) == bits(score[slot]) and fin == (status[slot] == br.DONE)
            want_state = frozen[slot] if fin else rt2.state_back(slot)
            assert np.array_equal(bits(rt.state_back(slot)), bits(want_state)), what + (slot, fin)
    # 4. every returned hypothesis's slot holds the replay's context for it: a DONE slot's as the step that ended it left it
    check_contexts(rt, ctxs, tables, [h[3] for grp in res for h in grp], what)
    print(what, "steps", run, "live rows changed", bitten, "contexts moved", moved, "ended", ended)
    return res, ctxs, frozen, bitten, ended, (kw, tables, tables2)


@pytest.mark.parametrize("v6", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("W,G", [(2, 1), (2, 2), (4, 1), (4, 2)])
def test_replay(ctx, made, v6, mode, W, G):
    for name in CONTEXTS:
        for alpha in (0.0, 1.0):
            for stop in (None, STOPS):
                res, ctxs, frozen, bitten, ended, (kw, tables, tables2) = replay(ctx, made, v6, mode, W, G, alpha, stop, name)
                assert bitten >= 1, (name, alpha, stop, "the context changed no live row's front")
                if stop is not None:
                    assert ended >= 1, (name, alpha, "the stop set ends no beam")
    # 4, the second half: a penalised greedy continuation from the slots (context `all`) equals the replay's from the host's contexts
    B = W * G
    rt, rt2, lb = made("rt", v6, B, 0), made("rt", v6, B, 1), made("bias")
    last = np.full(B, ALLOWED[0], np.uint32)
    states = np.zeros(B, np.uint32)
    for g in range(G):
        for toks, _, fin, slot in res[g]:
            last[slot] = toks[-1]
            states[slot] = ctxs[slot]["state"]
            if fin:
                rt2.state_load(frozen[slot], slot)
    load_contexts(ctxs, tables2[0], tables2[1])
    per_slot = lambda v: np.repeat(np.asarray(v), W) if np.ndim(v) else v
    go = dict(temperature=0.0, presence=per_slot(kw["presence"]), frequency=per_slot(kw["frequency"]), decay=0.99, mode=mode, logit_bias=lb,
              no_repeat_ngram=per_slot(kw["no_repeat_ngram"]), dry=tuple(per_slot(v) for v in kw["dry"]), dry_breakers=kw["dry_breakers"],
              grammar=tables[2])
    a, _ = rt.generate_penalized(last, 4, tables[0], window=tables[1], grammar_state=rt.last_grammar_state, **go)
    b, _ = rt2.generate_penalized(last, 4, tables2[0], window=tables2[1], grammar_state=states, **go)
    held = [slot for g in range(G) for _, _, _, slot in res[g]]
    assert np.array_equal(a[:, held], b[:, held])


# ----------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("v6,mode", [(False, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize("name", CONTEXTS)
def test_one_beam_is_the_greedy_call_with_the_context(ctx, made, v6, mode, name):
    G, W = 2, 1
    rt, lb = made("rt", v6, 2, 0), made("bias")
    kw, pars, tables = setup(made, name, G, W, 0)
    occ, win, g = tables
    zero_states(rt, G)
    start_contexts(kw, pars, tables, G, W)
    res, run = rt.generate_beam(FIRST, STEPS, 1, mode=mode, logit_bias=lb, **kw)
    beam_ctx = [(occ.back(q) if occ else None, win.back(q).tolist() if win else None, int(rt.last_grammar_state[q]) if g else None) for q in range(G)]
    zero_states(rt, G)
    start_contexts(kw, pars, tables, G, W)
    gk = {k: v for k, v in kw.items() if k != "occurrence"}
    if occ:
        tok, _ = rt.generate_penalized(FIRST, STEPS, occ, temperature=0.0, mode=mode, logit_bias=lb, **gk)
    else:
        tok, _ = rt.generate_greedy(FIRST, STEPS, mode=mode, logit_bias=lb, **gk)
    for q in range(G):
        (toks, _, finished, slot), = res[q]
        n = len(toks)           # a beam whose row the grammar empties dies; the greedy call goes on drawing
        assert slot == q and not finished and toks.tolist() == tok[:n, q].tolist(), (name, q)
        if n == STEPS:
            if occ:
                c, f = occ.back(q)
                assert np.array_equal(bits(c), bits(beam_ctx[q][0][0])) and np.array_equal(f, beam_ctx[q][0][1])
            if win:
                assert win.back(q).tolist() == beam_ctx[q][1]
            if g:
                assert int(rt.last_grammar_state[q]) == beam_ctx[q][2]
    assert any(len(res[q][0][0]) == STEPS for q in range(G)), "every beam died: the identity was not compared to the end"


def beam_words(rt, res):
    tok, par, sc = rt.last_beam_steps
    return ([[(t.tolist(), bits(np.float32(s)).tolist(), f, q) for t, s, f, q in grp] for grp in res], tok.tolist(), par.tolist(), bits(sc).tolist())


@pytest.mark.parametrize("v6", [False, True])
def test_an_empty_context_is_the_plain_call(ctx, made, v6):
    rt, lb = made("rt", v6, 4, 0), made("bias")
    zero_states(rt, 4)
    res, _ = rt.generate_beam(FIRST, 8, 2, stop=STOPS, length_penalty=1.0, logit_bias=lb)
    plain = beam_words(rt, res)
    gen, keep = wrk.GenerateOptions(), []
    wrk._fill_bias(gen, 2, keep, lb, None)
    ids, off = wrk._stop_csr(STOPS, 2, "groups")
    gen.stop_tokens, gen.stop_offsets = P_(ids, wrk._u32p), P_(off, wrk._u32p)
    for context in (None, wrk.BeamContext()):
        zero_states(rt, 4)
        out = raw_context(rt, FIRST, 8, 2, context, gen=gen, alpha=1.0, want=True)
        assert out == plain[1:]


# ----------------------------------------------------------------------------- 5. semantics
@pytest.mark.parametrize("v6", [False, True])
def test_semantics(ctx, made, v6):
    G, W, B = 2, 4, 8
    rt, lb = made("rt", v6, B, 0), made("bias")
    win, occ = made("win", B, 0), made("occ", B, 0)

    def fresh():
        zero_states(rt, B)
        for q in range(B):
            win.load(q, PROMPTS[q // W] if q % W == 0 else None)
            occ.load(q)
    for n in (2, 3):
        fresh()
        res, _ = rt.generate_beam(FIRST, STEPS, W, logit_bias=lb, window=win, no_repeat_ngram=n)
        for g in range(G):
            assert len(res[g]) == W
            for toks, _, _, slot in res[g]:
                assert not dry_ref.has_repeated_ngram(PROMPTS[g] + toks.tolist(), n), (n, g, toks)
                assert win.back(slot).tolist() == PROMPTS[g] + toks.tolist()
    fresh()
    res, _ = rt.generate_beam(FIRST, STEPS, W, logit_bias=lb, window=win)       # a window alone only records
    assert any(dry_ref.has_repeated_ngram(PROMPTS[g] + toks.tolist(), 2) for g in range(G) for toks, _, _, _ in res[g])
    # every hypothesis of a grammar call walks
    for kind in ("choices", "dense"):
        g_, starts = made(kind)
        fresh()
        res, _ = rt.generate_beam(FIRST, STEPS, W, logit_bias=lb, grammar=g_, grammar_state=starts)
        assert sum(len(grp) for grp in res) >= 1
        for g in range(G):
            for toks, _, _, slot in res[g]:
                assert g_.walk(starts[g], toks) == int(rt.last_grammar_state[slot]), (kind, g, toks)
    # a ban on slot gW alone holds for the whole group, and only for it
    fresh()
    plain, _ = rt.generate_beam(FIRST, STEPS, W, logit_bias=lb, occurrence=occ)
    t0 = int(plain[0][0][0][0])
    fresh()
    occ.ban(0, [t0])
    res, _ = rt.generate_beam(FIRST, STEPS, W, logit_bias=lb, occurrence=occ)
    assert all(t0 not in toks.tolist() for toks, _, _, _ in res[0])
    assert [h[0].tolist() for h in res[1]] == [h[0].tolist() for h in plain[1]]
    for toks, _, _, slot in res[0]:
        assert occ.back(slot)[1][t0] & wrk.Occurrence.BANNED


# ----------------------------------------------------------------------------- 6. validation
def raw_context(rt, first, steps, W, context, gen=None, alpha=0.0, mode=1, want=False):
    """wrk_v*_generate_beam_context below Runtime.generate_beam: the status code (want: the step arrays of a call that must succeed)"""
    ft = np.asarray(first, np.uint32)
    G = ft.size
    n = max(G * max(W, 1), 1)
    arr = dict(tokens=np.zeros(n * steps, np.uint32), lengths=np.zeros(n, np.uint32), scores=np.zeros(n, np.float32),
               finished=np.zeros(n, np.uint32), slots=np.zeros(n, np.uint32), num_hyps=np.zeros(G, np.uint32), steps_run=np.zeros(1, np.uint32),
               step_tokens=np.zeros((steps, n), np.uint32), step_parents=np.zeros((steps, n), np.uint32), step_scores=np.zeros((steps, n), np.float32))
    res = wrk.BeamResult(**{k: P_(v, wrk._f32p if v.dtype == np.float32 else wrk._u32p) for k, v in arr.items()})
    opt = wrk.BeamOptions(W, alpha, C.pointer(gen) if gen is not None else None)
    fn, mdl = rt._entry("generate_beam_context")
    ms = C.c_float()
    rc = fn(rt.ctx.h, mdl, rt.state, P_(ft, wrk._u32p), G, steps, C.byref(opt), C.byref(res), C.byref(ms), mode,
            C.byref(context) if context is not None else None)
    if not want:
        return rc
    assert rc == wrk.OK
    r = int(arr["steps_run"][0])
    return arr["step_tokens"][:r].tolist(), arr["step_parents"][:r].tolist(), bits(arr["step_scores"][:r]).tolist()


@pytest.mark.parametrize("v6", [False, True])
def test_argument_errors(ctx, made, v6):
    rt = made("rt", v6, 4, 0)
    occ, win = made("occ", 4, 0), made("win", 4, 0)
    g, _ = made("dense")
    keep = []

    def context(**kw):
        c = wrk.BeamContext()
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = P_(v, wrk._f32p if v.dtype == np.float32 else wrk._u32p)
            setattr(c, k, v)
        return c
    f = lambda x: np.full(2, x, np.float32)
    u = lambda x: np.full(2, x, np.uint32)
    zero = f(0.0)
    assert raw_context(rt, FIRST, 2, 2, context(occ=occ.h, presence=zero, frequency=zero, window=win.h, grammar=g.h)) == wrk.OK
    bad = []
    # arrays without their table, window or grammar
    bad.append(raw_context(rt, FIRST, 2, 2, context(presence=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(decay=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(no_repeat_ngram=u(2))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(dry_multiplier=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(num_dry_breakers=1)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(grammar_state=u(0))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(out_grammar_state=np.zeros(4, np.uint32))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(occ=occ.h)))                                            # a table without presence / frequency
    # a table, window or grammar of another context or vocabulary
    other = wrk.Context(0)
    o2, w2 = wrk.Occurrence(other, 4, V), wrk.TokenWindow(other, 4, V, 8)
    g2 = wrk.Grammar(other, V, g.token_class, g.transitions)
    bad.append(raw_context(rt, FIRST, 2, 2, context(occ=o2.h, presence=zero, frequency=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=w2.h)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(grammar=g2.h)))
    for x in (o2, w2, g2):
        x.close()
    other.close()
    o3, w3 = wrk.Occurrence(ctx, 4, V + 1), wrk.TokenWindow(ctx, 4, V + 1, 8)
    cls3, trans3 = wrk.grammar_from_dense(np.zeros((1, V + 1), np.int64))
    g3 = wrk.Grammar(ctx, V + 1, cls3, trans3)
    bad.append(raw_context(rt, FIRST, 2, 2, context(occ=o3.h, presence=zero, frequency=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=w3.h)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(grammar=g3.h)))
    # fewer than G * W slots
    o4, w4 = wrk.Occurrence(ctx, 3, V), wrk.TokenWindow(ctx, 3, V, 8)
    bad.append(raw_context(rt, FIRST, 2, 2, context(occ=o4.h, presence=zero, frequency=zero)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=w4.h)))
    for x in (o3, w3, g3, o4, w4):
        x.close()
    # values out of range
    for pres, freq, dec in ((f(np.nan), zero, None), (zero, f(np.inf), None), (zero, zero, f(1.5)), (zero, zero, f(-0.1))):
        bad.append(raw_context(rt, FIRST, 2, 2, context(occ=occ.h, presence=pres, frequency=freq, **({} if dec is None else dict(decay=dec)))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, dry_multiplier=f(-1.0))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, dry_base=f(0.5))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, dry_allowed_length=u(0))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, no_repeat_ngram=u(1))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, dry_breakers=u(V), num_dry_breakers=1)))
    bad.append(raw_context(rt, FIRST, 2, 2, context(window=win.h, num_dry_breakers=wrk.MAX_DRY_BREAKERS + 1, dry_breakers=np.zeros(32, np.uint32))))
    bad.append(raw_context(rt, FIRST, 2, 2, context(grammar=g.h, grammar_state=u(g.num_states))))           # a start state >= num_states
    # what stays refused, through `gen`: a sampler, stop sequences, log-probs, penalties / DRY / a grammar in gen itself; and lanes
    ok = context(window=win.h)

    def gen(**kw):
        o = wrk.GenerateOptions()
        for k, v in kw.items():
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = P_(v, wrk._f32p if v.dtype == np.float32 else wrk._u32p)
            setattr(o, k, v)
        return o
    one_f, one_u = np.ones(4, np.float32), np.ones(4, np.uint32)
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(temperature=one_f, top_p=one_f, seed=one_u)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(top_k=one_u)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(stop_seq_tokens=one_u, stop_seq_offsets=np.array([0, 1], np.uint32), stop_seq_owners=np.array([0, 1, 1], np.uint32))))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(out_logprob=one_f)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(num_top=1)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(presence=one_f)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(no_repeat_ngram=one_u)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, gen(grammar_state=one_u)))
    bad.append(raw_context(rt, FIRST, 2, 2, ok, mode=1 | (2 << 8)))
    assert bad == [wrk.E_ARG] * len(bad), bad
    assert raw_context(rt, FIRST, 2, 2, ok, gen(guidance_scale=one_f)) == wrk.E_UNSUPPORTED                # guidance


# ----------------------------------------------------------------------------- 7. the other loops are undisturbed
@pytest.mark.parametrize("v6,mode", [(False, 0), (False, 1), (True, 1)])
def test_other_loops_are_undisturbed(ctx, made, v6, mode):
    B = 4
    rt, lb = made("rt", v6, B, 0), made("bias")
    occ2 = wrk.Occurrence(ctx, B, V)
    four = [3, 88, 173, 258]

    def others():
        zero_states(rt, B)
        res, _ = rt.generate_beam(FIRST, 8, 2, stop=STOPS, length_penalty=1.0, mode=mode, logit_bias=lb)
        a = beam_words(rt, res)
        zero_states(rt, B)
        b, _ = rt.generate_greedy(four, 8, mode=mode)
        zero_states(rt, B)
        c, lens = rt.generate_stop(four, 8, STOPS, mode=mode, logit_bias=lb)
        zero_states(rt, B)
        for q in range(B):
            occ2.load(q)
        d, lens2 = rt.generate_stop(four, 8, STOPS, temperature=0.7, top_p=0.9, occurrence=occ2, presence=0.5, frequency=0.5, decay=0.99, mode=mode,
                                    logit_bias=lb)
        return a, b.tolist(), c.tolist(), lens.tolist(), d.tolist(), lens2.tolist()
    before = others()
    kw, pars, tables = setup(made, "all", 2, 2, 0)
    zero_states(rt, B)
    start_contexts(kw, pars, tables, 2, 2)
    rt.generate_beam(FIRST, 8, 2, stop=STOPS, length_penalty=1.0, mode=mode, logit_bias=lb, **kw)
    assert others() == before
    occ2.close()
