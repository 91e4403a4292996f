"""One step of beam search with a context per hypothesis in NumPy, worked from the contract of wrk_v7_generate_beam_context in
include/wrk_hip.h and composed from the rules the other tests already hold the kernels to: beam_ref (the selection),
penalty_ref, dry_ref, grammar_ref (the row stages and the updates) and logprob_ref (the candidate front).

A slot's context is a dict: counts f32 [V], flags u32 [V] (bit 0 present, bit 1 banned), window (list of ids, oldest first), state
(automaton state).  A group's parameters are a dict `par`: presence, frequency, decay, weights f32 [V] (occurrence; None: no table),
dry = dict(multiplier, base, allowed_length, no_repeat_ngram, breakers) and capacity (window; None: no window), grammar = (token_class,
transitions) (None: none).  One step:

  a. the row of slot b: the given row (head output, biased) -> penalize with slot b's counts / flags -> dry_row with slot b's window ->
     mask with slot b's state
  b. the candidate front (the W first tokens of that row in the sampler's order, with their log-probs) and beam_ref.select
  c. the context permutation by the step's copy list: every source is read before any destination is written; unlisted slots move
     nothing; the occurrence row moves whole, counts and both flag bits
  d. every slot filled in the step counts the token it was given in its own, post-permutation context: the occurrence update with the
     group's decay, the automaton advance, the window push.  Slots not filled are not touched

The keyword seams of `step` are what the mutants of tests/test_beam_ctx_ref.py replace.  Not a test module."""
import copy

import numpy as np

import beam_ref as br
import dry_ref
import grammar_ref
import logprob_ref
import penalty_ref

NO_TOKEN, NO_COPY = br.NO_TOKEN, br.NO_COPY


def new_context(V, state=0):
    return dict(counts=np.zeros(V, np.float32), flags=np.zeros(V, np.uint32), window=[], state=int(state))


def group_params(V, presence=None, frequency=None, decay=1.0, dry=None, capacity=None, grammar=None, weights=None):
    """presence / frequency None: no occurrence table; capacity None: no window; grammar None: none"""
    par = dict(occ=presence is not None or frequency is not None, presence=presence or 0.0, frequency=frequency or 0.0, decay=decay,
               weights=np.ones(V, np.float32) if weights is None else np.asarray(weights, np.float32), capacity=capacity,
               dry=dict(dry_ref.DEFAULTS, breakers=()), grammar=grammar)
    par["dry"].update(dry or {})
    return par


def context_row(row, c, par):
    """stage a: the row the candidate front of a slot with context `c` sees"""
    x = np.asarray(row, np.float32)
    if par["occ"]:
        x = penalty_ref.penalize(x, c["counts"], c["flags"], par["presence"], par["frequency"])
    if par["capacity"] is not None:
        d = par["dry"]
        x = dry_ref.dry_row(x, c["window"], d["multiplier"], d["base"], d["allowed_length"], d["no_repeat_ngram"], d["breakers"])
    if par["grammar"] is not None:
        x = grammar_ref.mask(x, par["grammar"][0], par["grammar"][1], c["state"])
    return x


def front(rows, W):
    """the W first tokens of every row in the sampler's order and their log-probs: (ids u32 [B][W], lp f32 [B][W])"""
    _, ids, lp = logprob_ref.top_rows(rows, np.zeros(len(rows), np.uint32), W)
    return ids.astype(np.uint32), lp.astype(np.float32)


def count_token(c, token, par):
    """stage d for one slot, in place"""
    if par["occ"]:
        c["counts"], c["flags"] = penalty_ref.update(c["counts"], c["flags"], int(token), par["weights"], par["decay"])
    if par["grammar"] is not None:
        c["state"] = grammar_ref.advance(par["grammar"][0], par["grammar"][1], c["state"], int(token))
    if par["capacity"] is not None:
        c["window"] = dry_ref.push(c["window"], int(token), par["capacity"])


def permute(ctxs, copy_src, move_flags=True, fused=False):
    """stage c: a gather of every listed source, then the scatter.  fused (a mutant): one pass in slot order, reading what it wrote"""
    out = ctxs if fused else [copy.deepcopy(c) for c in ctxs]
    src = ctxs if fused else [copy.deepcopy(c) for c in ctxs]
    for q, p in enumerate(copy_src):
        if p == NO_COPY:
            continue
        moved = copy.deepcopy(src[int(p)])
        if not move_flags:
            moved["flags"] = out[q]["flags"].copy()
        out[q] = moved
    return out


def step(rec, ctxs, rows, W, inv_norm, pars, stops=None, front=front, do_permute=True, update_first=False, update_unfilled=False,
         move_flags=True, fused=False):
    """rec = (score, key, length, status) [B]; ctxs: B contexts; rows [B][V]: the head output (biased); pars: one group_params per group.
    Returns (sel, contexts after the step, the rows of stage a).  The inputs are not modified."""
    B = len(ctxs)
    par_of = [pars[q // W] for q in range(B)]
    seen = np.stack([context_row(rows[q], ctxs[q], par_of[q]) for q in range(B)])
    ids, lp = front(seen, W)
    sel = br.select(rec[0], rec[1], rec[2], rec[3], ids, lp, W, inv_norm, stops)
    out = [copy.deepcopy(c) for c in ctxs]

    def update(cs):
        for q in range(B):
            if sel["token"][q] != NO_TOKEN:
                count_token(cs[q], sel["token"][q], par_of[q])
            elif update_unfilled:       # a mutant: an unfilled slot counts the token it goes on feeding -- here its last window entry or 0
                count_token(cs[q], cs[q]["window"][-1] if cs[q]["window"] else 0, par_of[q])
    if update_first:
        update(out)
    if do_permute:
        out = permute(out, sel["copy_src"], move_flags, fused)
    if not update_first:
        update(out)
    return sel, out, seen


def run(first_rows_of, G, W, steps, pars, start, stops=None, length_penalty=0.0, **seams):
    """The whole loop: first_rows_of(tokens [B], parents [B] or None) -> the head output rows [B][V] of feeding tokens[q] to slot q after
    moving the states by `parents` (slot q <- slot parents[q]; None at step 0).  start: the G groups' contexts of slot gW.  Returns
    (hypotheses per group by rank: (tokens, score, finished, slot), contexts, per-step (token, parent, score), changed) with changed
    the count of LIVE rows whose front differs from the front of the raw row."""
    B = G * W
    inv = br.inv_norm_table(length_penalty, steps)
    rec = br.start_records(G, W)
    V = len(start[0]["counts"])
    ctxs = [copy.deepcopy(start[q // W]) if q % W == 0 else new_context(V, start[q // W]["state"]) for q in range(B)]
    hist, changed, rows = [], 0, first_rows_of(None, None)
    for s in range(steps):
        sel, ctxs, seen = step(rec, ctxs, rows, W, inv, pars, stops, **seams)
        raw_ids, _ = front(np.asarray(rows, np.float32), W)
        seen_ids, _ = front(seen, W)
        changed += sum(int(rec[3][q] == br.LIVE and not np.array_equal(raw_ids[q], seen_ids[q])) for q in range(B))
        hist.append((sel["token"].copy(), sel["parent"].copy(), sel["score"].copy()))
        rec = (sel["score"], sel["key"], sel["length"], sel["status"])
        if not (rec[3] == br.LIVE).any():
            break
        if s + 1 < steps:
            rows = first_rows_of(sel["token"], sel["parent"])
    toks, pars_ = [h[0] for h in hist], [h[1] for h in hist]
    hyps = [[(br.backtrack(toks, pars_, q, int(rec[2][q])), float(rec[0][q]), bool(rec[3][q] == br.DONE), q) for q in grp]
            for grp in br.hypotheses(rec[1], rec[3], W)]
    return hyps, ctxs, hist, changed
