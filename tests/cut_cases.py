"""The rows and the parameter grid of the cut sampler's kernel test (tests/test_gpu_cut.py), shared with the CPU checks in
tests/test_cut_ref.py: that the rows leave at least 95 % of the cases of every V unambiguous, that the mutants differ on the grid, and
that the emulation of the kernel's arithmetic agrees with the restatement.  Not a test module."""
import functools

import numpy as np

import cut_ref as CR
import filter_cases as FC
from cut_ref import Cut

# 1, 2: degenerate rows; 50; both sides of every register variant's limit (1024, 4096, 8192 tokens) and the L2 path up to the vocabulary
VOCABS = (1, 2, 50, 1000, 1024, 1025, 4096, 4097, 8192, 8193, 65536)
TEMPS = (0.7, 1.5)
SEEDS = (1, 7)
STEP = 5
# (top_p, top_k, min_p): off, the preset the benchmark uses, each filter alone
FILTERS = ((1.0, 0, 0.0), (0.9, 40, 0.05), (1.0, 5, 0.0), (0.3, 0, 0.0), (1.0, 0, 0.5))
CUTS = (
    Cut(),
    Cut(top_n_sigma=1.0), Cut(top_n_sigma=2.5), Cut(top_n_sigma=np.inf),
    Cut(epsilon=3e-4), Cut(epsilon=0.02), Cut(epsilon=1.0),
    Cut(eta=3e-4), Cut(eta=0.05), Cut(eta=1.0),
    Cut(xtc_p=0.5, xtc_t=0.1), Cut(xtc_p=1.0, xtc_t=0.02), Cut(xtc_p=1.0, xtc_t=0.5), Cut(xtc_p=1.0, xtc_t=0.6), Cut(xtc_p=1.0, xtc_t=0.0),
    Cut(xtc_p=0.0, xtc_t=0.1),
    Cut(1.5, 1e-3, 1e-3, 0.7, 0.05), Cut(3.0, 0.0, 0.01, 1.0, 0.2),
)


def rows_for(V):
    """[(name, f32 logits)]: filter_cases' row kinds (V = 2 has them too: two logits each)."""
    return FC.rows_for(V)


def grid(V, salt=0):
    """[(T, top_p, top_k, min_p, Cut, seed)] of one row; every case gets a seed of its own."""
    out = []
    for c in CUTS:
        for p, k, m in FILTERS:
            for t in TEMPS:
                for s in SEEDS:
                    out.append((t, p, k, m, c, s + 16 * (len(out) + salt)))
    return out


@functools.lru_cache(maxsize=None)
def expected(V):
    """Per row kind: (name, logits, grid, wanted tokens with None where the case is ambiguous).  Computed once per V."""
    res = []
    for j, (name, l) in enumerate(rows_for(V)):
        row = CR.Row(l)
        g = grid(V, salt=1000 * j)
        want = [None if row.ambiguous(t, p, k, m, c, s, STEP) else row.sample(t, p, k, m, c, s, STEP) for t, p, k, m, c, s in g]
        res.append((name, l, g, want))
    return res


def columns(g):
    """The grid as the arrays `Context.sample_logits` takes."""
    f = np.float32
    return dict(temperature=np.array([c[0] for c in g], f), top_p=np.array([c[1] for c in g], f), top_k=np.array([c[2] for c in g], np.uint32),
                min_p=np.array([c[3] for c in g], f), top_n_sigma=np.array([c[4].top_n_sigma for c in g], f),
                epsilon_cutoff=np.array([c[4].epsilon for c in g], f), eta_cutoff=np.array([c[4].eta for c in g], f),
                xtc=(np.array([c[4].xtc_p for c in g], f), np.array([c[4].xtc_t for c in g], f)),
                seed=np.array([c[5] for c in g], np.uint32))
