"""NumPy (f64) restatement of the Mirostat v2 device sampler (wrk_sample_logits_mirostat / the decode loops' mirostat_tau, mirostat_eta,
mirostat_mu; Basu et al. 2021, Alg. 2; llama.cpp `mirostat_v2`), on top of tests/sampling_ref.py, whose row, order, u and greedy
branch it keeps:

  * tau == 0: the row is sampling_ref.sample's (top_p included) and mu is untouched;
  * T == 0 or an all -inf row: the greedy branch, mu untouched; top_p is not read by a Mirostat row;
  * w_i = exp((l_i - mx) / T), W = sum w, surprise s_i = log2 W - (l_i - mx) / T * log2 e;
  * candidates: rank 0 and every token with s_i <= mu -- a prefix of the sampler's order;
  * draw: the first rank whose cumulative weight reaches u * W_c, W_c = the candidates' weight;
  * observed surprise s = log2 W_c - (l_y - mx) / T * log2 e, then mu <- mu - eta * (s - tau); a fresh sequence starts at 2 tau.

Bounds (eps = 2^-24, the unit roundoff of f32; the device evaluates the expressions above in f32 with every sum that feeds a decision
in 2^40 fixed point):

  threshold.  The device compares fl(log2 W) - fl(fl(fl(l - mx) * fl(1 / T)) * log2e) with mu.  Near the threshold the product term is
  at most M = |mu| + log2 V in magnitude.  It carries five roundings (the subtraction, 1 / T, two products, the constant): 5 eps M.
  The final subtraction rounds once more: eps M.  log2 W: the fixed-point sum drops less than one unit of 2^-40 per token against
  W >= 1, expf is good to 2 ulp (4 eps relative on every term, so on W), the conversion to f32 rounds once: (V 2^-40 + 5 eps) log2 e;
  log2f returns 40 + log2 W <= 60 to one ulp of [32, 64), 2^-18.  `mu_slack` adds these up; a token whose surprise is that close to mu
  makes the candidate set ambiguous.  At mu = 20, V = 65 536 it is 1.8e-5 bits (the issue's CPU check used a flat 1e-4).

  mu.  One counted draw moves mu by -eta (s - tau) with s = fl(log2 W_c) - term: the same log2 error with W_c for W, the same 5 eps on
  the token's own term |x log2 e| = |s - log2 W_c|, then three roundings (s, s - tau, the product with eta: 3 eps |s - tau| eta in all,
  bounded with max(|s|, |tau|)) and the rounding of the new mu (eps |mu|).  `mu_tol` is that sum; over a call the bounds of the counted
  draws add up, and the accumulated bound widens the threshold slack of the following draws.

Not a test module: tests/test_mirostat_ref.py checks it, tests/test_gpu_mirostat.py holds the kernel to it.
"""
import numpy as np

import sampling_ref as S

EPS = 2.0 ** -24
LOG2E = 1.0 / np.log(2.0)


def _log2_err(V: int) -> float:
    """error of the device's log2 of a fixed-point weight sum over at most V tokens"""
    return (V * 2.0 ** -40 + 5 * EPS) * LOG2E + 2.0 ** -18


def mu_slack(mu: float, V: int) -> float:
    M = abs(mu) + np.log2(max(V, 2))
    return 6 * EPS * M + _log2_err(V)


def mu_tol(eta: float, tau: float, mu_new: float, s: float, log2_wc: float, V: int) -> float:
    term = abs(s - log2_wc)
    err_s = _log2_err(V) + 5 * EPS * term
    return eta * (err_s + 3 * EPS * (abs(s) + abs(tau))) + EPS * abs(mu_new)


class Row:
    """One row with what does not depend on (mu, u) computed once per temperature."""

    def __init__(self, logits, temperature: float):
        l = np.asarray(logits, np.float32)
        l = np.where(np.isnan(l), np.float32(-np.inf), l).astype(np.float64) + 0.0
        self.l, self.V, self.T = l, l.size, float(temperature)
        self.finite = bool((l > -np.inf).any())
        if self.T == 0.0 or not self.finite:
            return
        self.order = np.lexsort((np.arange(l.size), -l))
        mx = l.max()
        with np.errstate(invalid="ignore"):
            x = np.where(l == mx, 0.0, (l - mx) / self.T)[self.order]       # mx = +inf: the top tokens weigh 1, as on the device
        self.x = x
        self.w = np.exp(x)
        self.cw = np.cumsum(self.w)
        self.s = np.log2(self.cw[-1]) - x * LOG2E       # ascending along the order

    def count(self, mu: float) -> int:
        return max(1, int(np.searchsorted(self.s, mu, side="right")))

    def step(self, mu: float, tau: float, eta: float, seed=0, step=0, u=None):
        """(token, mu after the draw, (s, log2 W_c) or None when mu did not move)"""
        if self.T == 0.0 or not self.finite:
            return S.greedy(self.l), mu, None
        n = self.count(mu)
        u = S.uniform(seed, step) if u is None else u
        r = int(np.searchsorted(self.cw[:n] / self.cw[n - 1], u, side="left"))
        r = r if r < n else 0
        log2_wc = float(np.log2(self.cw[n - 1]))
        s = log2_wc - float(self.x[r]) * LOG2E
        return int(self.order[r]), mu - eta * (s - tau), (s, log2_wc)

    def ambiguous(self, mu: float, seed=0, step=0, extra: float = 0.0) -> bool:
        """The candidate set changes when mu moves by the f32 rounding the comparison can carry (plus `extra`, the bound mu itself has
        accumulated), or u lies within EDGE_SLACK of an edge of the draw."""
        if self.T == 0.0 or not self.finite:
            return False
        slack = mu_slack(mu, self.V) + extra
        if self.count(mu - slack) != self.count(mu + slack):
            return True
        n = self.count(mu)
        c = self.cw[:n] / self.cw[n - 1]
        u = S.uniform(seed, step)
        return bool(min(abs(u), np.min(np.abs(c - u))) < S.EDGE_SLACK)


def sample(logits, temperature, top_p, tau, eta, mu, seed=0, step=0, u=None):
    """(token, mu after the draw) of one row."""
    if tau == 0.0:
        return S.sample(logits, temperature, top_p, seed, step, u), mu
    tok, mu2, _ = Row(logits, temperature).step(mu, tau, eta, seed, step, u)
    return tok, mu2


def ambiguous(logits, temperature, top_p, tau, mu, seed=0, step=0) -> bool:
    if tau == 0.0:
        return S.ambiguous(logits, temperature, top_p, seed, step)
    return Row(logits, temperature).ambiguous(mu, seed, step)


def start_mu(tau):
    return 2.0 * tau


def sample32(logits, temperature, tau, eta, mu, seed=0, step=0, variant=None):
    """The device's evaluation restated in f32 / 2^40 fixed point (tau > 0, T > 0, a finite row): (token, mu after the draw).
    variant: a deliberately wrong reading of the contract, for the mutant tests -- "sign", "norm" (surprise against W, not W_c)."""
    f = np.float32
    l = np.asarray(logits, f)
    l = (np.where(np.isnan(l), f(-np.inf), l) + f(0.0)).astype(f)
    mx = l.max()
    top = int(np.flatnonzero(l == mx)[0])
    inv_t = f(1.0) / f(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(l == mx, f(0.0), ((l - mx).astype(f) * inv_t).astype(f)).astype(f)
        e = np.where(l == mx, f(1.0), np.exp(x.astype(np.float64)).astype(f))
    fixed = (e.astype(np.float64) * 2.0 ** 40).astype(np.uint64)      # e * 2^40 is exact in f32 and in f64
    log2_w = f(np.log2(np.float64(f(float(fixed.sum()))))) - f(40.0)
    s_all = (log2_w - (x * f(LOG2E)).astype(f)).astype(f)
    cand = s_all <= f(mu)
    cand[top] = True
    order = np.lexsort((np.arange(l.size), -l.astype(np.float64)))
    order = order[cand[order]]
    cw = np.cumsum(fixed[order].astype(object))
    wc = int(cw[-1])
    U = S.splitmix(seed, step) >> 40
    target = -((-U * wc) >> 24)        # ceil(U * W_c / 2^24)
    r = next(i for i, c in enumerate(cw) if c >= target)
    y = int(order[r])
    denom = fixed.sum() if variant == "norm" else wc
    s = (f(np.log2(np.float64(f(float(denom))))) - f(40.0)) - (x[y] * f(LOG2E)).astype(f)
    step_ = f(eta) * (f(s) - f(tau))
    return y, float(f(mu) + step_ if variant == "sign" else f(mu) - step_)
