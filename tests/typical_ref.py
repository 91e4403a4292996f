"""NumPy (f64) restatement of the locally typical device sampler (wrk_sample_logits_typical / the decode loops' typical_p; Meister et
al. 2022; HF `TypicalLogitsWarper`, llama.cpp `typical_p`), on top of tests/sampling_ref.py, whose row, order, u and greedy branch it
keeps:

  * typical_p >= 1: the row is sampling_ref.sample's (top_p included);
  * T == 0 or an all -inf row: the greedy branch; top_p is not read by a typical row;
  * p = softmax(l) at temperature 1, g_i = mx - l_i, gbar = sum p_i g_i (a -inf logit adds 0), d_i = |g_i - gbar| (= |-ln p_i - H|;
    +inf for a -inf logit);
  * typical order: d ascending, ties by index ascending; the token at rank r of it is in iff the mass before it is <= typical_p (the
    token that crosses is in, rank 0 always);
  * the draw is among the candidates in the sampler's order with weights p^(1/T) and sampling_ref's u.

Bounds (eps = 2^-24).  The device sums e = exp(l - mx) and e g in 2^40 fixed point and divides once.
  GBAR_SLACK.  expf is good to 2 ulp (4 eps relative), g = fl(mx - l) and the product e g round once each: the two sums are off by at
  most 4 eps and 6 eps relative, their quotient by 10 eps gbar; gbar <= ln V < 14 for V <= 2^20: 8.4e-6.  Truncation drops less than
  one unit of 2^-40 per token from either sum against a denominator >= 1: V 2^-40 (1 + gbar) <= 1.5e-5 at V = 2^20, 9e-7 at 65 536.
  The quotient's own rounding and the two roundings of d = |fl(fl(mx - l) - gbar)| at g <= 32: 3 eps 32 = 5.7e-6.  `gbar_slack(V)`
  is their sum, 1.5e-5 at V = 65 536 (the issue's CPU check used 2e-5).  Two tokens whose d differ by less than twice the slack may
  swap places in the typical order (on opposite sides of gbar by the error of gbar, on one side when f32 collapses their g).
  The prefix mass against typical_p: sampling_ref.PREFIX_SLACK, as for the nucleus -- the same fixed-point sums and the same
  floor(P * total) comparison.

Not a test module: tests/test_typical_ref.py checks it, tests/test_gpu_typical.py holds the kernel to it.
"""
import numpy as np

import sampling_ref as S

EPS = 2.0 ** -24


def gbar_slack(V: int) -> float:
    return 10 * EPS * 14.0 + V * 2.0 ** -40 * 15.0 + 3 * EPS * 32.0


class Row:
    """One row with what does not depend on (typical_p, T, u) computed once.  signed / typical_order_draw: deliberately wrong readings
    of the contract, for the mutant tests (d without the absolute value; the draw made in typical order)."""

    def __init__(self, logits, signed=False, crossing_out=False, typical_order_draw=False):
        l = np.asarray(logits, np.float32)
        l = np.where(np.isnan(l), np.float32(-np.inf), l).astype(np.float64) + 0.0
        self.l, self.V = l, l.size
        self.finite = bool((l > -np.inf).any())
        self.crossing_out, self.typical_order_draw = crossing_out, typical_order_draw
        if not self.finite:
            return
        self.mx = mx = l.max()
        with np.errstate(invalid="ignore"):
            g = np.where(l == mx, 0.0, mx - l)
        e = np.exp(-g)
        self.p = e / e.sum()
        self.gbar = float(np.sum(np.where(e > 0.0, self.p * np.where(np.isinf(g), 0.0, g), 0.0)))
        self.g = g
        self.d = g - self.gbar if signed else np.abs(g - self.gbar)
        self.torder = np.lexsort((np.arange(l.size), self.d))
        ps = self.p[self.torder]
        self.before = np.cumsum(ps) - ps
        self.sorder = np.lexsort((np.arange(l.size), -l))

    def count(self, typical_p: float) -> int:
        n = int(np.count_nonzero(self.before <= typical_p))
        return max(1, n - 1 if self.crossing_out else n)

    def candidates(self, temperature: float, typical_p: float):
        """(candidate tokens in the sampler's order, running sums of their normalised weights)"""
        n = self.count(typical_p)
        if self.typical_order_draw:
            toks = self.torder[:n]
        else:
            inside = np.zeros(self.V, bool)
            inside[self.torder[:n]] = True
            toks = self.sorder[inside[self.sorder]]
        with np.errstate(invalid="ignore"):
            w = np.exp(np.where(self.l[toks] == self.mx, 0.0, (self.l[toks] - self.mx) / temperature))
        c = np.cumsum(w)
        return toks, c / c[-1]

    def sample(self, temperature, top_p, typical_p, seed=0, step=0, u=None) -> int:
        if typical_p >= 1.0:
            return S.sample(self.l, temperature, top_p, seed, step, u)
        if temperature == 0.0:
            return S.greedy(self.l)
        if not self.finite:
            return 0
        toks, c = self.candidates(temperature, typical_p)
        u = S.uniform(seed, step) if u is None else u
        r = int(np.searchsorted(c, u, side="left"))
        return int(toks[r] if r < toks.size else toks[0])

    def ambiguous(self, temperature, top_p, typical_p, seed=0, step=0) -> bool:
        """A prefix mass of the typical order within PREFIX_SLACK of typical_p; a token of another logit whose d lies within twice
        gbar_slack of the crossing token's (the last candidate's): only a swap with that token changes the set -- tokens that trade
        places among the ranks before it leave the same tokens before it, and so the same masses at and after it; u within EDGE_SLACK
        of an edge."""
        if typical_p >= 1.0:
            return S.ambiguous(self.l, temperature, top_p, seed, step)
        if temperature == 0.0 or not self.finite:
            return False
        if np.any(np.abs(self.before[1:] - typical_p) < S.PREFIX_SLACK):
            return True
        n = self.count(typical_p)
        if n < self.V:
            cross = self.torder[n - 1]
            close = (np.abs(self.d - self.d[cross]) < 2.0 * gbar_slack(self.V)) & (self.l != self.l[cross])
            if close.any():
                return True
        _, c = self.candidates(temperature, typical_p)
        u = S.uniform(seed, step)
        return bool(min(abs(u), np.min(np.abs(c - u))) < S.EDGE_SLACK)


def sample(logits, temperature, top_p, typical_p, seed=0, step=0, u=None) -> int:
    return Row(logits).sample(temperature, top_p, typical_p, seed, step, u)


def ambiguous(logits, temperature, top_p, typical_p, seed=0, step=0) -> bool:
    return Row(logits).ambiguous(temperature, top_p, typical_p, seed, step)


def sample32(logits, temperature, typical_p, seed=0, step=0) -> int:
    """The device's evaluation restated in f32 / 2^40 fixed point (typical_p < 1, T > 0, a finite row)."""
    f = np.float32
    l = np.asarray(logits, f)
    l = (np.where(np.isnan(l), f(-np.inf), l) + f(0.0)).astype(f)
    mx = l.max()
    idx = np.arange(l.size)
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.where(l == mx, f(0.0), (mx - l).astype(f)).astype(f)
        e = np.where(l == mx, f(1.0), np.exp(-g.astype(np.float64)).astype(f)).astype(f)
        eg = np.where((l > -np.inf) & (e > 0), (e * g).astype(f), f(0.0)).astype(f)
    fe = (e.astype(np.float64) * 2.0 ** 40).astype(np.uint64)
    feg = (eg.astype(np.float64) * 2.0 ** 40).astype(np.uint64)
    gbar = f(float(feg.sum()) / float(fe.sum()))
    d = np.abs((g - gbar).astype(f))
    torder = np.lexsort((idx, d.astype(np.float64)))
    mass = fe[torder].astype(object)
    before = np.cumsum(mass) - mass
    total = int(mass.sum())
    target = int(np.floor(float(f(typical_p)) * float(total)))
    n = max(1, sum(1 for b in before if b <= target))
    inside = np.zeros(l.size, bool)
    inside[torder[:n]] = True
    sorder = np.lexsort((idx, -l.astype(np.float64)))
    toks = sorder[inside[sorder]]
    inv_t = f(1.0) / f(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(l[toks] == mx, f(0.0), ((l[toks] - mx).astype(f) * inv_t).astype(f))
        w = np.where(l[toks] == mx, f(1.0), np.exp(x.astype(np.float64)).astype(f))
    cw = np.cumsum((w.astype(np.float64) * 2.0 ** 40).astype(np.uint64).astype(object))
    U = S.splitmix(seed, step) >> 40
    tgt = -((-U * int(cw[-1])) >> 24)
    return int(toks[next(i for i, c in enumerate(cw) if c >= tgt)])
