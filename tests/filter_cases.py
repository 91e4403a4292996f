"""The rows and the parameter grid of the filtered sampler's kernel test (tests/test_gpu_filter.py), shared with the CPU check in
tests/test_filter_ref.py that the rows leave at least 95 % of the cases of every V unambiguous.  Not a test module."""
import numpy as np

import filter_ref as F

VOCABS = (1, 50, 1000, 3000, 16384, 65529, 65536)
MIN_PS = (0.0, 0.02, 0.5, 1.0)
TOP_PS = (0.3, 0.9, 1.0)
TEMPS = (0.5, 1.0, 2.0)
SEEDS = (1, 7)
STEP = 5


def top_ks(V):
    return (0, 1, 2, 5, 40, V - 1, V, V + 7, 2 ** 32 - 1)


def rows_for(V):
    """[(name, f32 logits)]: the row kinds of test_gpu_sampling.py -- flat (V <= 1000) or a plateau, peaked, half-masked, duplicated."""
    rng = np.random.default_rng(V)
    if V <= 1000:
        flat = rng.normal(0.0, 0.5, V)
        peaked = rng.normal(0.0, 3.0, V); peaked[rng.integers(V)] += 12.0
        masked = rng.normal(0.0, 2.0, V); masked[rng.random(V) < 0.5] = -np.inf; masked[rng.integers(V)] = 1.0
        dup = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0
        rows = [("flat", flat), ("peaked", peaked), ("masked", masked), ("dup", dup)]
    else:
        head = rng.choice(V, 24, replace=False)
        plateau = rng.normal(0.0, 0.3, V); plateau[rng.choice(V, 200, replace=False)] += 12.0   # a flat head on a flat floor
        peaked = rng.normal(0.0, 2.0, V); peaked[head] += rng.normal(14.0, 1.0, head.size)
        masked = peaked.copy(); masked[rng.random(V) < 0.5] = -np.inf; masked[head] = peaked[head]
        dup = np.round(rng.normal(0.0, 2.0, V) * 2.0) / 2.0; dup[head] = np.round(rng.normal(14.0, 1.0, head.size))
        rows = [("plateau", plateau), ("peaked", peaked), ("masked", masked), ("dup", dup)]
    return [(n, l.astype(np.float32)) for n, l in rows]


def grid(V, salt=0):
    """[(T, top_p, top_k, min_p, seed)] of one row; every case gets a seed of its own."""
    out = []
    for k in top_ks(V):
        for m in MIN_PS:
            for p in TOP_PS:
                for t in TEMPS:
                    for s in SEEDS:
                        out.append((t, p, k, m, s + 16 * (len(out) + salt)))
    return out


def expected(V):
    """Per row kind: (name, logits, grid, wanted tokens with None where the case is ambiguous).  Computed once per V."""
    res = []
    for j, (name, l) in enumerate(rows_for(V)):
        row = F.Row(l)
        g = grid(V, salt=1000 * j)
        want = [None if row.ambiguous(t, p, k, m, s, STEP) else row.sample(t, p, k, m, s, STEP) for t, p, k, m, s in g]
        res.append((name, l, g, want))
    return res
