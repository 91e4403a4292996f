"""NumPy restatement of constrained decoding (web-rwkv-gguf_amd/csrc/wrk_grammar.hip): a deterministic automaton over
token ids with alphabet compression.

  * token_class [V] maps every token to a class, transitions [S][C] holds the next state or REJECT;
  * mask: a row in state s keeps the bits of every logit whose token is allowed in s and gets -inf elsewhere;
  * advance: a drawn token moves the state to transitions[s][class]; a rejected token leaves it where it was;
  * a constrained pick is the existing pick (sampling_ref / filter_ref / mirostat_ref / typical_ref, after penalty_ref) on the masked row.

Not a test module: tests/test_grammar_ref.py checks it and the table builders of the package, tests/test_gpu_grammar.py holds the kernels
and the decode loops to it.
"""
import numpy as np

import filter_ref as F
import mirostat_ref as M
import sampling_ref as S
import typical_ref as T

REJECT = 0xFFFF


def allowed(cls, trans, s: int) -> np.ndarray:
    """bool [V]: the tokens allowed in state s"""
    return np.asarray(trans)[int(s)][np.asarray(cls, np.int64)] != REJECT


def mask(row, cls, trans, s: int) -> np.ndarray:
    """The row as the pick sees it in state s: the source bits where the token is allowed, the bits of -inf elsewhere."""
    bits = np.asarray(row, np.float32).view(np.uint32)
    return np.where(allowed(cls, trans, s), bits, np.uint32(0xFF800000)).astype(np.uint32).view(np.float32)


def advance(cls, trans, s: int, token: int) -> int:
    nx = int(np.asarray(trans)[int(s)][int(cls[int(token)])])
    return int(s) if nx == REJECT else nx


def walk(cls, trans, s: int, tokens) -> int:
    """The state after `tokens`; ValueError at the first rejected one."""
    for i, t in enumerate(tokens):
        nx = int(np.asarray(trans)[int(s)][int(cls[int(t)])])
        if nx == REJECT:
            raise ValueError(f"token {i} (id {int(t)}) is not allowed in state {s}")
        s = nx
    return int(s)


def expand(cls, trans) -> np.ndarray:
    """The dense table [S][V] of next states, -1 for REJECT: the inverse of grammar_from_dense."""
    t = np.asarray(trans, np.int64)[:, np.asarray(cls, np.int64)]
    return np.where(t == REJECT, -1, t)


def accepts(cls, trans, start: int, tokens) -> bool:
    try:
        walk(cls, trans, start, tokens)
        return True
    except ValueError:
        return False


def random_dense(rng, S: int, V: int, columns: int, lo: float = 1 / 3, hi: float = 1 / 2) -> np.ndarray:
    """A random table [S][V] with at most `columns` distinct columns in which every state allows between lo and hi of the tokens (at
    least one)."""
    proto = np.full((S, columns), -1, np.int64)
    col = rng.integers(0, columns, V)
    col[:min(columns, V)] = rng.permutation(min(columns, V))            # every column in use while V allows
    for s in range(S):
        for _ in range(64):
            on = rng.random(columns) < rng.uniform(lo, hi)
            share = on[col].mean()
            if on.any() and (columns < 8 or lo * 0.9 <= share <= hi * 1.1):
                break
        if not on[col].any():
            on[col[0]] = True
        proto[s, on] = rng.integers(0, S, int(on.sum()))
    return proto[:, col]


# ----------------------------------------------------------------------------- the picks of the decode loops on a masked row
class Pick:
    """One sequence's pick parameters, as the decode loops take them: family in {"greedy", "sample", "filter", "mirostat", "typical"}."""

    def __init__(self, family, temperature=1.0, top_p=1.0, seed=0, top_k=0, min_p=0.0, tau=0.0, eta=0.0, mu=None, typical_p=1.0):
        self.family, self.t, self.p, self.seed = family, float(np.float32(temperature)), float(np.float32(top_p)), int(seed)
        self.top_k, self.min_p, self.tau, self.eta, self.typ = int(top_k), float(np.float32(min_p)), float(np.float32(tau)), float(np.float32(eta)), float(np.float32(typical_p))
        self.mu = M.start_mu(self.tau) if mu is None else float(mu)
        self.tol, self.lost = 0.0, False        # Mirostat: the bound mu has accumulated; whether an ambiguous step has been met

    def draw(self, row, step: int):
        """(token, ambiguous) of the pick on `row` (already penalised and masked) at sampler step `step`; a Mirostat pick moves mu."""
        if self.family == "greedy":
            return S.greedy(row), False
        if self.family == "sample":
            return S.sample(row, self.t, self.p, self.seed, step), S.ambiguous(row, self.t, self.p, self.seed, step)
        if self.family == "filter":
            r = F.Row(row)
            args = (self.t, self.p, self.top_k, self.min_p, self.seed, step)
            return r.sample(*args), r.ambiguous(*args)
        if self.family == "typical":
            r = T.Row(row)
            args = (self.t, self.p, self.typ, self.seed, step)
            return r.sample(*args), r.ambiguous(*args)
        if self.family == "mirostat":
            if self.tau == 0.0:
                return S.sample(row, self.t, self.p, self.seed, step), S.ambiguous(row, self.t, self.p, self.seed, step)
            r = M.Row(row, self.t)
            # once a step is ambiguous the device's mu may have gone another way: the rest of the sequence is excused, as in
            # test_gpu_mirostat.py's replay; until then the threshold slack is widened by the bound mu has accumulated
            if self.lost or r.ambiguous(self.mu, self.seed, step, extra=self.tol):
                self.lost = True
                return r.step(self.mu, self.tau, self.eta, self.seed, step)[0], True
            tok, self.mu, info = r.step(self.mu, self.tau, self.eta, self.seed, step)
            if info:
                self.tol += M.mu_tol(self.eta, self.tau, self.mu, info[0], info[1], r.V)
            return tok, False
        raise ValueError(self.family)


def loop(rows_of, cls, trans, state: int, pick: Pick, steps: int, penalise=None):
    """The reference loop of one sequence: rows_of(step, tokens so far) -> the raw logits row of the step; penalise(row, tokens so far)
    -> the penalised row (None: no penalties).  Returns (tokens, ambiguous flags, final state)."""
    toks, amb = [], []
    for i in range(steps):
        row = rows_of(i, toks)
        if penalise:
            row = penalise(row, toks)
        t, a = pick.draw(mask(row, cls, trans, state), i)
        toks.append(t)
        amb.append(a)
        state = advance(cls, trans, state, t)
    return toks, amb, state
