"""The rows and the parameter grids of the Mirostat and typical kernel tests (tests/test_gpu_mirostat.py, tests/test_gpu_typical.py),
shared with the CPU checks that the rows leave at least 95 % of the cases of every V unambiguous.  Not a test module.

V: 1, 50, 1000 (one register element per thread), 3000 (four), 6000 (eight), 16 384, 65 529 and 65 536 (rows re-read from L2, the odd
tail included).  Rows: the peaked / masked / dup kinds of filter_cases.rows_for at every V, and a row on a 1/4 grid.  A dense flat row
and a plateau row are left out: their typical boundary falls among tokens whose d differ by less than f32 can order, and their prefix
masses lie closer together than PREFIX_SLACK (tests keep a flat row for the distribution only)."""
import functools

import numpy as np

import mirostat_ref as M
import typical_ref as TY

VOCABS = (1, 50, 1000, 3000, 6000, 16384, 65529, 65536)
TEMPS = (0.5, 1.0, 2.0)
MUS = (0.5, 2.0, 5.0, 10.0, 20.0)
TYPICAL_PS = (0.2, 0.5, 0.9, 0.95, 1.0)
SEEDS = (3, 11)
STEP = 5
TAU, ETA = 5.0, 0.1
TOP_P = 0.7         # read by the off rows only


def rows_for(V):
    """[(name, f32 logits)]: a head of up to 24 likely tokens on a floor -- continuous, half-masked, on a 1/2 grid, on a 1/4 grid -- so that
    the cuts of the grids below fall among tokens that f32 can tell apart, as the filtered sampler's peaked rows do."""
    rng = np.random.default_rng(1000 + V)
    head = rng.choice(V, min(24, max(1, V // 4)), replace=False)
    peaked = rng.normal(0.0, 2.0, V); peaked[head] += rng.normal(14.0, 1.0, head.size)
    masked = peaked.copy(); masked[rng.random(V) < 0.5] = -np.inf; masked[head] = peaked[head]
    dup = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0; dup[head] = np.round(rng.normal(14.0, 1.0, head.size))
    quarter = np.round(rng.normal(0.0, 2.5, V) * 4.0) / 4.0; quarter[head] = np.round(rng.normal(13.0, 1.5, head.size) * 4.0) / 4.0
    return [(n, l.astype(np.float32)) for n, l in (("peaked", peaked), ("masked", masked), ("dup", dup), ("quarter", quarter))]


def grid(values, salt=0):
    """[(T, value, seed)]: every case gets a seed of its own."""
    out = []
    for v in values:
        for t in TEMPS:
            for s in SEEDS:
                out.append((t, v, s + 16 * (len(out) + salt)))
    return out


@functools.lru_cache(maxsize=None)
def mirostat_expected(V):
    """Per row kind: (name, logits, grid of (T, mu, seed), [(token, mu after, tolerance) or None where the case is ambiguous])."""
    res = []
    for j, (name, l) in enumerate(rows_for(V)):
        g = grid(MUS, salt=500 * j)
        rows = {t: M.Row(l, t) for t in TEMPS}
        want = []
        for t, mu, s in g:
            if rows[t].ambiguous(mu, s, STEP):
                want.append(None)
                continue
            tok, mu2, (sur, lw) = rows[t].step(mu, TAU, ETA, s, STEP)
            want.append((tok, mu2, M.mu_tol(ETA, TAU, mu2, sur, lw, V)))
        res.append((name, l, g, want))
    return res


@functools.lru_cache(maxsize=None)
def typical_expected(V):
    """Per row kind: (name, logits, grid of (T, typical_p, seed), [token or None where the case is ambiguous])."""
    res = []
    for j, (name, l) in enumerate(rows_for(V)):
        g = grid(TYPICAL_PS, salt=700 * j)
        row = TY.Row(l)
        want = [None if row.ambiguous(t, TOP_P, p, s, STEP) else row.sample(t, TOP_P, p, s, STEP) for t, p, s in g]
        res.append((name, l, g, want))
    return res
