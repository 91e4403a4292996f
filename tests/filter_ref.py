"""NumPy restatement of the filtered device sampler (wrk_sample_logits_filtered / the decode loops' top_k and min_p), on top of
tests/sampling_ref.py, whose contract it keeps:

  * order: logit descending, ties by index ascending, NaN as -inf, -0 as +0 (sampling_ref's);
  * the candidates are the first n = min(n_P, n_K, n_M) ranks of that order;
  * n_P: sampling_ref's nucleus count against the whole row's softmax mass (not renormalised after the other cuts); top_p >= 1: V;
  * n_K: top_k, or V when top_k is 0 or >= V; top_k == 1 is the greedy branch (as T == 0 or top_p == 0);
  * n_M: the number of tokens with fl32(l - mx) >= fl32(ln(min_p)), mx the row max, the subtraction in f32, ln(min_p) taken in f64 of
    the f32 min_p and rounded once to f32; min_p == 0: V.  Rank 0 always passes (l == mx), also when mx = +inf;
  * weights p^(1/T) inside the candidates; draw, u, seed and step exactly sampling_ref's.

The top-k and the min-p cut are exact (an integer count, an f32 comparison restated bit for bit): they add no ambiguous cases.

Not a test module: tests/test_filter_ref.py checks it by hand-worked cases, tests/test_gpu_filter.py holds the kernel to it.
"""
import numpy as np

import sampling_ref as S


def ln_min_p(min_p) -> np.float32:
    """What the kernel receives: fl32(ln(min_p)) with the logarithm in f64, -inf for "off"."""
    m = np.float64(np.float32(min_p))
    with np.errstate(divide="ignore"):
        return np.float32(np.log(m))


def clean32(logits) -> np.ndarray:
    """The row as the kernel reads it: f32, NaN -> -inf, -0 -> +0."""
    l = np.asarray(logits, np.float32)
    l = np.where(np.isnan(l), np.float32(-np.inf), l)
    return (l + np.float32(0.0)).astype(np.float32)


def top_k_count(top_k: int, V: int) -> int:
    return V if top_k == 0 or top_k >= V else int(top_k)


def min_p_count(logits, min_p) -> int:
    if float(np.float32(min_p)) == 0.0:
        return int(np.asarray(logits).size)
    l = clean32(logits)
    mx = l.max()
    with np.errstate(invalid="ignore"):
        d = (l - mx).astype(np.float32)
        ok = (l == mx) | (d >= ln_min_p(min_p))
    return int(np.count_nonzero(ok))


class Row:
    """One row with everything that does not depend on the parameters computed once (the GPU test asks for hundreds of parameter sets
    per row): the order, the masses before every rank, and per temperature the running weight sums over the whole order."""

    def __init__(self, logits):
        self.l64 = clean32(logits).astype(np.float64)
        self.V = self.l64.size
        with np.errstate(all="ignore"):
            self.order, _, self.before = S.nucleus(self.l64, 1.0, 1.0)
        self.finite = bool((self.l64 > -np.inf).any())
        self._cw = {}
        self._nm = {}

    def counts(self, top_p: float, top_k: int, min_p: float):
        n_p = self.V if top_p >= 1.0 else int(np.count_nonzero(self.before <= top_p))
        key = float(np.float32(min_p))
        if key not in self._nm:
            self._nm[key] = min_p_count(self.l64.astype(np.float32), min_p)
        return n_p, top_k_count(top_k, self.V), self._nm[key]

    def cum_weights(self, temperature: float) -> np.ndarray:
        if temperature not in self._cw:
            with np.errstate(invalid="ignore"):
                w = np.exp((self.l64[self.order] - self.l64.max()) / temperature)
            self._cw[temperature] = np.cumsum(np.where(np.isnan(w), 1.0, w))     # mx = +inf: the top tokens weigh 1, as on the device
        return self._cw[temperature]

    def greedy_case(self, temperature, top_p, top_k) -> bool:
        return temperature == 0.0 or top_p == 0.0 or top_k_count(top_k, self.V) == 1

    def candidates(self, temperature, top_p, top_k=0, min_p=0.0):
        """(tokens of the candidate set in rank order, running sums of their normalised weights)."""
        n = min(self.counts(top_p, top_k, min_p))
        cw = self.cum_weights(temperature)[:n]
        return self.order[:n], cw / cw[-1]

    def sample(self, temperature, top_p, top_k=0, min_p=0.0, seed=0, step=0, u=None) -> int:
        if self.greedy_case(temperature, top_p, top_k):
            return S.greedy(self.l64)
        if not self.finite:
            return 0
        toks, c = self.candidates(temperature, top_p, top_k, min_p)
        u = S.uniform(seed, step) if u is None else u
        r = int(np.searchsorted(c, u, side="left"))       # the first rank with u <= c[r]
        return int(toks[r] if r < toks.size else toks[0])

    def ambiguous(self, temperature, top_p, top_k=0, min_p=0.0, seed=0, step=0) -> bool:
        """sampling_ref.ambiguous on the filtered candidates: a prefix mass within PREFIX_SLACK of P at a rank where it can change n
        (a rank the other two cuts drop anyway excuses nothing), or u within EDGE_SLACK of an edge of the draw over the candidates."""
        if self.greedy_case(temperature, top_p, top_k) or not self.finite:
            return False
        n_p, n_k, n_m = self.counts(top_p, top_k, min_p)
        if top_p < 1.0:
            reach = min(n_k, n_m) + 1
            if np.any(np.abs(self.before[:reach] - top_p) < S.PREFIX_SLACK):
                return True
        _, c = self.candidates(temperature, top_p, top_k, min_p)
        u = S.uniform(seed, step)
        return bool(min(abs(u), np.min(np.abs(c - u))) < S.EDGE_SLACK)


def candidates(logits, temperature, top_p, top_k=0, min_p=0.0):
    """(tokens of the candidate set in rank order, their normalised weights)."""
    toks, c = Row(logits).candidates(temperature, top_p, top_k, min_p)
    return toks, np.diff(np.concatenate([[0.0], c]))


def sample(logits, temperature, top_p, top_k=0, min_p=0.0, seed=0, step=0, u=None) -> int:
    return Row(logits).sample(temperature, top_p, top_k, min_p, seed, step, u)


def ambiguous(logits, temperature, top_p, top_k=0, min_p=0.0, seed=0, step=0) -> bool:
    return Row(logits).ambiguous(temperature, top_p, top_k, min_p, seed, step)
