"""tests/beam_ctx_ref.py -- one step of beam search with a context per hypothesis -- against groups worked by hand, the
mutants those groups must reject, and the shape the GPU tests run, checked on the oracle's logits.

The hand-worked groups use V = 8 and rows that are -30 everywhere but at a few tokens, so every log-prob below is one of
  lp(5 vs 4)   = -log(1 + e^-1)   = -0.3133 / -1.3133        lp(5 vs 4.5) = -0.4741 / -0.9741        lp(10 vs 0 or less) = -0.0000 / <= -9
and the order of a group's candidates can be read off the scores.

The chosen shape (test_chosen_shape_on_the_oracle): oracle/rwkv7.py's tiny model (seed 42) with the vocabulary narrowed to the six
tokens range(3, 512, 85) by a bias set that bans the rest -- on the raw tiny model the random logits almost never repeat a token in 12
steps and a context would change nothing -- first tokens 3 and 88, 12 steps, G = 2, W in {2, 4}.  With this module's reference (f64
log-softmax rounded to f32, not the kernels' bit rule) every condition holds on this allowed set.  The test also asserts what the GPU
test asserts per configuration -- the context changes the front of at least one live row -- and prints the count: 10 to 72 live rows per
run here (W = 2: 10 / 30 / 30 for the ban, the penalties and both; W = 4: 34 / 64 / 72)."""
import functools

import numpy as np
import pytest

import beam_ctx_ref as bc
import beam_ref as br
import dry_ref
import penalty_ref
from oracle import gguf as ogguf
from oracle import rwkv7 as orwkv7
from oracle import synth

V = 8
NO = br.NO_TOKEN
NC = br.NO_COPY
REJ = 0xFFFF


def row(**at):
    x = np.full(V, -30.0, np.float32)
    for k, v in at.items():
        x[int(k[1:])] = v
    return x


def ctx_with(window=(), counts=None, banned=(), state=0):
    c = bc.new_context(V, state)
    c["window"] = list(window)
    for t, n in (counts or {}).items():
        c["counts"][t] = n
        c["flags"][t] |= penalty_ref.PRESENT
    for t in banned:
        c["flags"][t] |= penalty_ref.BANNED
    return c


def records(score, status, length=None, key=None):
    score = np.asarray(score, np.float32)
    return (score, score.copy() if key is None else np.asarray(key, np.float32),
            np.asarray([3] * len(status) if length is None else length, np.uint32), np.asarray(status, np.uint32))


WINDOW = dict(capacity=8)
BAN2 = dict(capacity=8, dry=dict(no_repeat_ngram=2))


# every case: (name, W, records, contexts, rows, params, stops) -> want = dict(token, parent, copy_src, and per slot what its context
# must hold afterwards)
def case_swap():
    """two beams whose n-gram bans differ trade places: slot 0's window (1 2 1) bans 2, slot 1's (3 4 3) bans 4.  Candidates: (1, 0)
    0 - 0.4741, (0, 5) -0.6 - 0.0001, (1, 7) -0.9741, (0, 6) about -9.6: slot 0 takes slot 1's child and slot 1 slot 0's"""
    rec = records([-0.6, 0.0], [br.LIVE, br.LIVE])
    ctxs = [ctx_with([1, 2, 1]), ctx_with([3, 4, 3])]
    rows = [row(t2=10, t5=9, t6=0), row(t4=10, t0=5, t7=4.5)]
    want = dict(token=[0, 5], parent=[1, 0], copy_src=[1, 0], window=[[3, 4, 3, 0], [1, 2, 1, 5]])
    return "swap", 2, rec, ctxs, rows, bc.group_params(V, **BAN2), (), want


def case_broadcast():
    """the start of a call: slot 0 LIVE with token 1 counted once, slot 1 DEAD.  presence = frequency = 0.5 take 1 from token 1's 5.0, so
    the front is 2 (4.8) then 1 (4.0); both children come from slot 0 and each counts only its own token"""
    rec = records([0.0, -np.inf], [br.LIVE, br.DEAD], length=[0, 0])
    ctxs = [ctx_with(counts={1: 1.0}), ctx_with(counts={6: 3.0})]
    rows = [row(t1=5.0, t2=4.8, t3=1.0), row(t0=1.0)]
    want = dict(token=[2, 1], parent=[0, 0], copy_src=[NC, 0], counts=[{1: 1.0, 2: 1.0}, {1: 2.0}])
    return "broadcast", 2, rec, ctxs, rows, bc.group_params(V, presence=0.5, frequency=0.5), (), want


def case_chain():
    """three LIVE beams, windows (5), (6), (7) that only record.  Candidates: (1, 0) 0, (2, 1) -0.1 - 0.3133, (2, 2) -0.1 - 1.3133, slot
    0's best -10: slot 0 <- slot 1, slot 1 <- slot 2, slot 2 keeps its own"""
    rec = records([-10.0, 0.0, -0.1], [br.LIVE] * 3)
    ctxs = [ctx_with([5]), ctx_with([6]), ctx_with([7])]
    rows = [row(t3=1.0), row(t0=10.0), row(t1=5.0, t2=4.0)]
    want = dict(token=[0, 1, 2], parent=[1, 2, 2], copy_src=[1, 2, NC], window=[[6, 0], [7, 1], [7, 2]])
    return "chain", 3, rec, ctxs, rows, bc.group_params(V, **WINDOW), (), want


def case_done_pushed_out_of_three():
    """three slots, slot 0 DONE with key -20.  Candidates: (1, 0) -1 - 0.3133, (1, 1) -1 - 1.3133, (2, 3) -10, the DONE slot -20: it is
    pushed out, slot 0 takes slot 1's first child and slot 1 its second, and slot 2 keeps its own"""
    rec = records([0.0, -1.0, -10.0], [br.DONE, br.LIVE, br.LIVE], key=[-20.0, -1.0, -10.0])
    ctxs = [ctx_with([5]), ctx_with([6]), ctx_with([7])]
    rows = [row(t0=1.0), row(t0=5.0, t1=4.0), row(t3=10.0)]
    want = dict(token=[0, 1, 3], parent=[1, 1, 2], copy_src=[1, NC, NC], window=[[6, 0], [6, 1], [7, 3]])
    return "pushed-out DONE, broadcast", 3, rec, ctxs, rows, bc.group_params(V, **WINDOW), (), want


def case_done_stays():
    """slot 0 is DONE with key -1 and window (5 5); slot 1 LIVE at -0.2.  Candidates: (1, 0) -0.5133, the DONE slot -1, (1, 1) -1.5133:
    the DONE slot stays and nothing touches its context; slot 1 keeps its own and counts token 0"""
    rec = records([-1.0, -0.2], [br.DONE, br.LIVE])
    ctxs = [ctx_with([5, 5], counts={5: 2.0}), ctx_with([6], counts={6: 1.0})]
    rows = [row(t7=3.0), row(t0=5.0, t1=4.0)]
    want = dict(token=[NO, 0], parent=[0, 1], copy_src=[NC, NC], window=[[5, 5], [6, 0]], counts=[{5: 2.0}, {6: 1.0, 0: 1.0}])
    return "DONE stays", 2, rec, ctxs, rows, bc.group_params(V, presence=0.0, frequency=0.0, **WINDOW), (), want


def case_done_pushed_out():
    """the same with the DONE slot's key at -5: both of slot 1's children beat it, slot 0 is reused and its context overwritten"""
    rec = records([-5.0, -0.2], [br.DONE, br.LIVE])
    ctxs = [ctx_with([5, 5], counts={5: 2.0}), ctx_with([6], counts={6: 1.0})]
    rows = [row(t7=3.0), row(t0=5.0, t1=4.0)]
    want = dict(token=[0, 1], parent=[1, 1], copy_src=[1, NC], window=[[6, 0], [6, 1]], counts=[{6: 1.0, 0: 1.0}, {6: 1.0, 1: 1.0}])
    return "DONE pushed out", 2, rec, ctxs, rows, bc.group_params(V, presence=0.0, frequency=0.0, **WINDOW), (), want


def grammar():
    """state 0 allows 0 (-> 0) and 1 (-> 1); state 1 allows only 3 (-> 0)"""
    trans = np.full((2, V), REJ, np.uint16)
    trans[0, 0], trans[0, 1], trans[1, 3] = 0, 1, 0
    return np.arange(V, dtype=np.uint16), trans


def case_grammar_empties_a_row():
    """slot 1 is in state 1, whose only token 3 the row holds at -inf (a bias ban): the masked row has no finite logit, slot 1 gives no
    candidate and both places go to slot 0's children 0 and 1, whose states are 0 and 1"""
    rec = records([-3.0, 0.0], [br.LIVE, br.LIVE])
    ctxs = [ctx_with(state=0), ctx_with(state=1)]
    r1 = row(t0=9.0, t4=8.0)
    r1[3] = -np.inf
    rows = [row(t0=5.0, t1=4.0, t2=20.0), r1]
    want = dict(token=[0, 1], parent=[0, 0], copy_src=[NC, 0], state=[0, 1])
    return "grammar empties a row", 2, rec, ctxs, rows, bc.group_params(V, grammar=grammar()), (), want


def case_one_beam():
    """W = 1: the window (1 2 1) bans 2 and the beam takes 4"""
    rec = records([0.0], [br.LIVE])
    want = dict(token=[4], parent=[0], copy_src=[NC], window=[[1, 2, 1, 4]])
    return "W = 1", 1, rec, [ctx_with([1, 2, 1])], [row(t2=10.0, t4=5.0)], bc.group_params(V, **BAN2), (), want


CASES = [case_swap, case_broadcast, case_chain, case_done_pushed_out_of_three, case_done_stays, case_done_pushed_out, case_grammar_empties_a_row,
         case_one_beam]


def holds(case, **seams):
    """whether the step gives what the case wants"""
    name, W, rec, ctxs, rows, par, stops, want = case()
    sel, out, _ = bc.step(rec, ctxs, rows, W, br.inv_norm_table(0.0, 8), [par], [list(stops)], **seams)
    ok = sel["token"].tolist() == want["token"] and sel["parent"].tolist() == want["parent"] and sel["copy_src"].tolist() == want["copy_src"]
    for q, c in enumerate(out):
        if "window" in want:
            ok = ok and c["window"] == want["window"][q]
        if "state" in want:
            ok = ok and c["state"] == want["state"][q]
        if "counts" in want:
            full = np.zeros(V, np.float32)
            for t, n in want["counts"][q].items():
                full[t] = n
            ok = ok and np.array_equal(c["counts"], full) and np.array_equal((c["flags"] & 1) != 0, full != 0)
    return bool(ok)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_hand_worked_groups(case):
    assert holds(case)


def two_steps_with_a_ban(**seams):
    """bans follow a hypothesis: token 2 is banned in slot 0 alone (occ.ban before the call).  Step 0 (slot 1 DEAD) puts slot 0's
    children 0 and 1 in slots 0 and 1; in step 1 both rows offer 2 at 10.0 and neither child may take it"""
    par = bc.group_params(V, presence=0.0, frequency=0.0)
    ctxs = [ctx_with(banned=[2]), ctx_with()]
    inv = br.inv_norm_table(0.0, 8)
    sel, ctxs, _ = bc.step(br.start_records(1, 2), ctxs, [row(t2=10.0, t0=5.0, t1=4.0), row()], 2, inv, [par], **seams)
    first = sel["token"].tolist()
    rec = (sel["score"], sel["key"], sel["length"], sel["status"])
    sel, ctxs, _ = bc.step(rec, ctxs, [row(t2=10.0, t3=1.0, t4=-2.0), row(t2=10.0, t3=1.0, t4=-2.0)], 2, inv, [par], **seams)
    return first, sel["token"].tolist(), [bool(c["flags"][2] & penalty_ref.BANNED) for c in ctxs]


def test_bans_follow_a_hypothesis():
    first, second, banned = two_steps_with_a_ban()
    assert first == [0, 1] and 2 not in second and banned == [True, True]
    # lp(1 vs -2) = -0.0486 / -3.0486: (0, 3) -0.3133 - 0.0486, (1, 3) -1.3133 - 0.0486, (0, 4) -0.3133 - 3.0486
    assert second == [3, 3]


MUTANTS = {
    "no context permutation": dict(do_permute=False),
    "update before permutation": dict(update_first=True),
    "update of unfilled slots": dict(update_unfilled=True),
    "flags not moved": dict(move_flags=False),
    "gather and scatter fused": dict(fused=True),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutants_are_rejected(name):
    seams = MUTANTS[name]
    failed = [c.__name__ for c in CASES if not holds(c, **seams)]
    ban = two_steps_with_a_ban(**seams)
    if ban != ([0, 1], [3, 3], [True, True]):
        failed.append("bans")
    assert failed, name
    # and each by the group that was written for it
    need = {"no context permutation": "case_swap", "update before permutation": "case_broadcast", "update of unfilled slots": "case_done_stays",
            "flags not moved": "bans", "gather and scatter fused": "case_swap"}[name]
    assert need in failed, (name, failed)


# ----------------------------------------------------------------------------- the chosen shape on the oracle's logits
ALLOWED = list(range(3, 512, 85))
FIRST = [3, 88]
STEPS = 12


@functools.lru_cache(maxsize=None)
def tiny():
    return orwkv7.build_v7(ogguf.GgufReader(synth.make_v7_gguf(synth.CONFIGS["tiny"], 42)), weights_f16=False)


def oracle_beam(W, pars, **seams):
    """the reference loop on the oracle's tiny model with the six-token bias; returns (hypotheses, changed rows)"""
    G, Vm = len(FIRST), synth.CONFIGS["tiny"].num_vocab
    B = G * W
    rt = orwkv7.V7Runtime(tiny(), B, act_f16=True)
    cur = np.repeat(np.asarray(FIRST, np.int64), W)
    banned = np.ones(Vm, bool)
    banned[ALLOWED] = False

    def rows_of(tokens, parents):
        if tokens is not None:
            rt.state.data = rt.state.data[:, np.asarray(parents, np.int64)].copy()
            cur[tokens != NO] = tokens[tokens != NO]
        logits = rt.infer_chunk([[int(t)] for t in cur], list(range(B)))
        return np.where(banned[None, :], np.float32(-np.inf), logits.astype(np.float32))
    start = [bc.new_context(Vm) for _ in range(G)]
    hyps, _, _, changed = bc.run(rows_of, G, W, STEPS, pars, start, **seams)
    return hyps, changed


@functools.lru_cache(maxsize=None)
def shape_runs(W):
    Vm = synth.CONFIGS["tiny"].num_vocab
    mk = lambda **kw: [bc.group_params(Vm, **kw) for _ in FIRST]
    confs = dict(none=mk(), ban2=mk(capacity=64, dry=dict(no_repeat_ngram=2)), ban3=mk(capacity=64, dry=dict(no_repeat_ngram=3)),
                 pen=mk(presence=0.5, frequency=0.5), both=mk(presence=0.5, frequency=0.5, capacity=64, dry=dict(no_repeat_ngram=2)))
    ref = {k: oracle_beam(W, p) for k, p in confs.items()}
    mut = {k: oracle_beam(W, confs[k], do_permute=False) for k in ("ban2", "pen", "both")}
    return ref, mut


@pytest.mark.parametrize("W", [2, 4])
def test_chosen_shape_on_the_oracle(W):
    ref, mut = shape_runs(W)
    toks = lambda run: [[h[0] for h in grp] for grp in run[0]]
    assert all(dry_ref.has_repeated_ngram(t, 2) for grp in toks(ref["none"]) for t in grp)
    assert not any(dry_ref.has_repeated_ngram(t, 2) for grp in toks(ref["ban2"]) for t in grp)
    assert not any(dry_ref.has_repeated_ngram(t, 3) for grp in toks(ref["ban3"]) for t in grp)
    for k in ("ban2", "pen", "both"):
        print(W, k, "live rows whose front the context changed:", ref[k][1])
        assert ref[k][1] >= 1, (k, ref[k][1])
        for g in range(len(FIRST)):
            assert toks(ref[k])[g] != toks(mut[k])[g], (W, k, g)
