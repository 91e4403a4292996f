"""Beam search's step rule in NumPy with f32 scalars, worked from the contract of wrk_v7_generate_beam in include/wrk_hip.h -- not from
web-rwkv-gguf_amd/csrc/wrk_beam_select.h, which the tests compare with this.

A group is W slots, each a record (score f32, key f32, length, status).  One step (the header's numbered clauses):
  1. every LIVE slot b gives its W first tokens in the sampler's order with their log-probs; a token whose lp is -inf or NaN is no
     candidate; candidate (b, j): raw = f32(score_b + lp), len = length_b + 1, key = f32(raw * inv_norm[len])
  2. every DONE slot gives one candidate, itself, with the key it got when it ended
  3. order: key descending, ties by slot of origin ascending, then j ascending; the first W survive
  4. a surviving DONE slot stays where it is; the other slots, ascending, take the surviving live candidates in their order; slots
     left over become DEAD with score and key -inf and length 0
  5. a placed candidate (p, j): score = raw, key = key, length = len, feeds t_{p,j}; DONE if the token is in the stop set, else LIVE
  6. per slot: the token fed next (NO_TOKEN: not filled), the parent (itself when not filled), the copy source (NO_COPY when not
     filled or when the parent is the slot itself)
"""
import numpy as np

DEAD, LIVE, DONE = 0, 1, 2
NO_TOKEN = NO_COPY = 0xFFFFFFFF
NEG_INF = np.float32(-np.inf)


def inv_norm_table(length_penalty, max_len):
    """inv_norm[l] = float(1.0 / pow((double)l, (double)length_penalty)) for 1 <= l <= max_len; entry 0 is never read"""
    t = np.ones(max_len + 1, np.float32)
    for l in range(1, max_len + 1):
        t[l] = np.float32(1.0 / (float(l) ** float(length_penalty)))
    return t


def make_key(raw, inv_norm, n):
    return np.float32(np.float32(raw) * np.float32(inv_norm[n]))


def select_group(score, key, length, status, ids, lp, inv_norm, stop=(), make_key=make_key, order=None, done_stays=True):
    """One group's step.  score / key / length / status: [W]; ids / lp: [W][W] (row b only read when slot b is LIVE).  Returns a dict of
    [W] arrays: score, key (f32), length, status, token, parent (within the group), ended, copy_src (within the group, NO_COPY).
    make_key / order / done_stays: the seams the mutants of tests/test_beam_ref.py replace."""
    W = len(status)
    cands = []      # (key, origin, j, raw, len, token or None)
    for b in range(W):
        if status[b] == DONE:
            cands.append((np.float32(key[b]), b, 0, np.float32(score[b]), int(length[b]), None))
        if status[b] != LIVE:
            continue
        for j in range(W):
            x = np.float32(lp[b][j])
            if np.isnan(x) or x == NEG_INF:
                continue
            raw = np.float32(np.float32(score[b]) + x)
            n = int(length[b]) + 1
            cands.append((make_key(raw, inv_norm, n), b, j, raw, n, int(ids[b][j])))
    if order is None:
        order = lambda c: (-float(c[0]), c[1], c[2])        # a f32 key is exact in a double; -0 == +0
    surv = sorted(cands, key=order)[:W]
    out = dict(score=np.full(W, NEG_INF, np.float32), key=np.full(W, NEG_INF, np.float32), length=np.zeros(W, np.uint32),
               status=np.full(W, DEAD, np.uint32), token=np.full(W, NO_TOKEN, np.uint32), parent=np.arange(W, dtype=np.uint32),
               ended=np.zeros(W, np.uint32), copy_src=np.full(W, NO_COPY, np.uint32))
    taken = [False] * W
    movers = []
    for c in surv:
        if c[5] is None and done_stays:
            b = c[1]
            out["score"][b], out["key"][b], out["length"][b], out["status"][b] = score[b], key[b], length[b], DONE
            taken[b] = True
        else:
            movers.append(c)
    q = 0
    for k, o, j, raw, n, tok in movers:
        while taken[q]:
            q += 1
        taken[q] = True
        if tok is None:         # only a mutant moves a DONE slot
            out["score"][q], out["key"][q], out["length"][q], out["status"][q] = raw, k, n, DONE
            out["parent"][q] = o
            continue
        is_stop = tok in set(int(s) for s in stop)
        out["score"][q], out["key"][q], out["length"][q] = raw, k, n
        out["status"][q] = DONE if is_stop else LIVE
        out["token"][q], out["parent"][q], out["ended"][q] = tok, o, int(is_stop)
        if o != q:
            out["copy_src"][q] = o
    return out


def select(score, key, length, status, ids, lp, W, inv_norm, stops=None, **kw):
    """`select_group` over G = B / W groups of consecutive slots; parents and copy sources as slot indices of the whole batch.
    ids / lp: [B][W]; stops: one id list per group, or None."""
    B = len(status)
    assert B % W == 0
    outs = []
    for g in range(B // W):
        s = slice(g * W, (g + 1) * W)
        o = select_group(score[s], key[s], length[s], status[s], ids[s], lp[s], inv_norm, () if stops is None else stops[g], **kw)
        o["parent"] = o["parent"] + np.uint32(g * W)
        o["copy_src"] = np.where(o["copy_src"] == NO_COPY, np.uint32(NO_COPY), o["copy_src"] + np.uint32(g * W)).astype(np.uint32)
        outs.append(o)
    return {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}


def start_records(G, W):
    """the records a call starts with: slot gW LIVE with score 0, key 0 and length 0, the others DEAD"""
    score, key = np.full(G * W, NEG_INF, np.float32), np.full(G * W, NEG_INF, np.float32)
    length, status = np.zeros(G * W, np.uint32), np.full(G * W, DEAD, np.uint32)
    score[::W], key[::W], status[::W] = 0.0, 0.0, LIVE
    return score, key, length, status


def hypotheses(key, status, W):
    """per group the non-DEAD slots by key descending, ties by slot"""
    out = []
    for g in range(len(status) // W):
        qs = [q for q in range(g * W, (g + 1) * W) if status[q] != DEAD]
        out.append(sorted(qs, key=lambda q: (-float(key[q]), q)))
    return out


def backtrack(step_tokens, step_parents, slot, length):
    """the tokens of the hypothesis that ends in `slot`, through the parents of the steps that ran"""
    toks, cur = [], slot
    for s in range(len(step_tokens) - 1, -1, -1):
        if len(toks) == length:
            break
        t = int(step_tokens[s][cur])
        if t != NO_TOKEN:
            toks.append(t)
        cur = int(step_parents[s][cur])
    return toks[::-1]
