"""NumPy (f64) restatement of the cut sampler (wrk_sample_logits_cut / the decode loops' top_n_sigma, epsilon_cutoff, eta_cutoff and xtc;
DESIGN.md §7t), on top of tests/sampling_ref.py and tests/filter_ref.py, whose contract it keeps:

  * the row, the order and u: sampling_ref's -- NaN as -inf, -0 as +0, logit descending with ties by index ascending,
    u = (SplitMix64((seed << 32) | step) >> 40) * 2^-24;
  * p is the WHOLE row's softmax at temperature 1, never renormalised after another cut (llama.cpp renormalises over the survivors
    before XTC: a recorded divergence);
  * the candidates are the ranks [m0, n) of the order;
  * n = min(n_P, n_K, n_M, n_S, n_E, n_H); n_P, n_K, n_M are filter_ref's; each new count is a prefix with rank 0 always in:
      n_S = #{l >= max - top_n_sigma * sigma}, sigma the population standard deviation of the row's finite logits; fewer than two
            finite logits, or a +inf in the row: sigma = 0, the ties of the maximum stay.  top_n_sigma <= 0: off; +inf counts as the
            largest finite f32;
      n_E = #{p >= epsilon_cutoff}; 0: off;
      n_H = #{p >= min(eta_cutoff, sqrt(eta_cutoff) * exp(-H))}, H = -sum p ln p in nats (a -inf logit adds 0); 0: off;
  * XTC: m = #{p >= xtc_threshold}, m' = min(m, n).  The row's coin is the SECOND output of the SplitMix64 stream whose first output
    gives u: with s = (seed << 32) | step the generator's state after one output is s + G, after two s + 2 G (G = 0x9E3779B97F4A7C15),
    and c = (mix(s + 2 G) >> 40) * 2^-24, mix being SplitMix64's output function (`coin` below).  m' >= 2 and c < xtc_probability:
    m0 = m' - 1, every candidate at or above the threshold goes except the least likely of them; else m0 = 0.  xtc_probability == 0
    or xtc_threshold > 0.5: off.  [m0, n) is never empty;
  * weights p^(1/T) inside the candidates; the token drawn is the first rank of [m0, n) whose cumulative weight reaches u * W_c;
  * T == 0, top_p == 0 and top_k == 1 are the greedy branch: sampling_ref.greedy, no cut, no coin;
  * the parameters are f32 values; with all five off every token is filter_ref's.

What the kernel computes, and the bound within which it may decide a comparison the other way (derived as tests/ops_ref.py derives
its bounds: every rounding step of the kernel's arithmetic bounded by its unit roundoff u = 2^-24 times the magnitude it rounds, the
fixed-point truncations by their step).  With d = l - max (one f32 subtraction, error <= u |d|):

  * ln S: S = sum e in 2^40 fixed point -- every term's expf within 2 ulp (2^-22 relative) and truncated by at most 2^-40, so S is
    within 2^-22 S + V 2^-40 (S >= 1); logf of a value below 2^60 rounds within ulp(64) / 2 = 2^-18, and the subtraction of ln 2^40
    once more: |ln S error| <= 2^-22 + 2^-20 + 2^-18 + 2^-18 < LN_S_ERR = 2^-16;
  * epsilon: d >= fl(ln eps) + ln S against the exact ln p >= ln eps:  B_E = LN_S_ERR + 2^-22 (|d| + |ln eps| + |ln S|);
  * eta: H = ln S + gbar, gbar = sum e g / sum e from the same fixed point (numerator within 2^-22 of itself + V 2^-40, g rounded
    once), then two f32 roundings of values up to H: |H error| <= LN_S_ERR + 2^-21 (1 + H), and
    B_H = 2 LN_S_ERR + 2^-21 (1 + |d| + |ln eta| + H + |ln S|);
  * XTC: compared as ln p >= ln t, the same expression as epsilon: B_X = LN_S_ERR + 2^-22 (|d| + |ln t| + |ln S|), a relative bound
    on p against the threshold; and the coin is excused within one f32 ulp of xtc_probability (the comparison itself is exact: the
    coin is a 24-bit integer times 2^-24);
  * sigma: q = trunc(fl(g * fl(2^21 / span))), span = max - (smallest finite logit), is within 2 units of g 2^21 / span, so the
    quantised logits are within span 2^-20 of the true ones and their standard deviation, exact in integers, within span 2^-20 of
    sigma (the deviation is 1-Lipschitz in the sup norm); three more f32 roundings of sigma-sized values and one of the product:
    B_S = top_n_sigma (span 2^-20 + 2^-22 sigma) + 2^-23 |d|.

A case is ambiguous when a token within reach -- at a rank no other cut has dropped -- has its tested quantity within the bound of its
threshold, when the coin is within one ulp of xtc_probability, or when filter_ref's nucleus / draw slacks apply.

Not a test module: tests/test_cut_ref.py checks it by hand-worked cases, tests/test_gpu_cut.py holds the kernel to it.
"""
import collections

import numpy as np

import filter_ref as F
import sampling_ref as S

Cut = collections.namedtuple("Cut", "top_n_sigma epsilon eta xtc_p xtc_t", defaults=(0.0, 0.0, 0.0, 0.0, 0.0))
OFF = Cut()
FLT_MAX = float(np.finfo(np.float32).max)
LN_S_ERR = 2.0 ** -16
_GAMMA = 0x9E3779B97F4A7C15


def coin(seed: int, step: int) -> float:
    """The row's second uniform: SplitMix64's output function on the state advanced twice."""
    z = ((((seed & 0xFFFFFFFF) << 32) | (step & 0xFFFFFFFF)) + 2 * _GAMMA) & S._MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & S._MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & S._MASK
    return float((z ^ (z >> 31)) >> 40) * 2.0 ** -24


def f32(x) -> float:
    return float(np.float32(x))


def normal(cut) -> Cut:
    """The parameters as f32 values, +inf sigmas clamped, XTC off folded into probability 0."""
    c = Cut(*cut)
    ns = min(f32(c.top_n_sigma), FLT_MAX)
    xp, xt = f32(c.xtc_p), f32(c.xtc_t)
    return Cut(ns, f32(c.epsilon), f32(c.eta), 0.0 if xt > 0.5 else xp, xt)


def is_off(cut) -> bool:
    c = normal(cut)
    return c.top_n_sigma <= 0.0 and c.epsilon == 0.0 and c.eta == 0.0 and c.xtc_p == 0.0


def ln(x: float) -> float:
    with np.errstate(divide="ignore"):
        return float(np.log(np.float64(x)))


class Row(F.Row):
    """filter_ref.Row with the row statistics of the cuts: p in rank order, sigma, H."""

    def __init__(self, logits):
        super().__init__(logits)
        l = self.l64
        self.mx = l.max() if self.V else -np.inf
        fin = np.isfinite(l)
        with np.errstate(all="ignore"):
            e = np.exp(l - self.mx)
            e = np.where(np.isnan(e), 1.0, e)              # mx = +inf: the +inf tokens weigh 1, as on the device
            self.lnS = float(np.log(e.sum())) if self.finite else 0.0
            self.d = np.where(l == self.mx, 0.0, l - self.mx)[self.order]   # l - max in rank order, 0 at the ties of the maximum
        self.lnp = self.d - self.lnS                       # ln p in rank order, -inf for a -inf logit
        p = np.exp(self.lnp)
        with np.errstate(all="ignore"):
            self.H = float(-(p[p > 0] * self.lnp[p > 0]).sum())
        self.sigma = float(np.std(l[fin])) if fin.sum() >= 2 and self.mx < np.inf else 0.0
        self.sample_sigma = float(np.std(l[fin], ddof=1)) if fin.sum() >= 2 and self.mx < np.inf else 0.0     # a mutant's, never the contract's
        self.span = float(self.mx - l[fin].min()) if fin.any() and self.mx < np.inf else 0.0

    # ---- the pieces a mutant of tests/test_cut_ref.py replaces
    def sigma_of(self) -> float:
        return self.sigma

    def eta_ln(self, eta: float) -> float:
        """ln of min(eta, sqrt(eta) exp(-H))."""
        return min(ln(eta), 0.5 * ln(eta) - self.H)

    def xtc_count(self, cut, n: int) -> int:
        """m: the tokens with p >= xtc_threshold, p the whole row's (n, the upper count, is not read)."""
        return int(np.count_nonzero(self.lnp >= ln(normal(cut).xtc_t)))

    def xtc_first(self, m: int) -> int:
        """m0 of a row whose coin fell: all of the first m' = m ranks go but the last."""
        return m - 1

    def coin_of(self, seed: int, step: int) -> float:
        return coin(seed, step)

    def cut_counts(self, cut):
        """(n_S, n_E, n_H)."""
        c = normal(cut)
        V = self.V
        n_s = V if c.top_n_sigma <= 0.0 else max(1, int(np.count_nonzero(-self.d <= c.top_n_sigma * self.sigma_of())))
        n_e = V if c.epsilon == 0.0 else max(1, int(np.count_nonzero(self.lnp >= ln(c.epsilon))))
        n_h = V if c.eta == 0.0 else max(1, int(np.count_nonzero(self.lnp >= self.eta_ln(c.eta))))
        return n_s, n_e, n_h

    def upper(self, top_p, top_k, min_p, cut) -> int:
        return min(self.counts(top_p, top_k, min_p) + self.cut_counts(cut))

    def span_of(self, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0, c=None):
        """(m0, n): the candidates are ranks [m0, n)."""
        cut = normal(cut)
        n = self.upper(top_p, top_k, min_p, cut)
        m0 = 0
        if cut.xtc_p > 0.0:
            m = min(self.xtc_count(cut, n), n)
            c = self.coin_of(seed, step) if c is None else c
            if m >= 2 and c < cut.xtc_p:
                m0 = self.xtc_first(m)
        return m0, n

    def candidates(self, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0, c=None):
        """(tokens of the candidate set in rank order, running sums of their normalised weights)."""
        m0, n = self.span_of(temperature, top_p, top_k, min_p, cut, seed, step, c)
        if m0 == 0:         # filter_ref's own expression: with the cuts off the tokens are its tokens, bit for bit
            cw = self.cum_weights(temperature)[:n]
            return self.order[:n], cw / cw[-1]
        # weights relative to rank m0, the heaviest candidate (differences of the running sums over the whole order would cancel)
        lc = self.l64[self.order[m0:n]]
        with np.errstate(invalid="ignore"):
            w = np.exp((lc - lc[0]) / temperature)
        cw = np.cumsum(np.where(np.isnan(w), 1.0, w))       # rank m0 at +inf or -inf: its ties weigh 1, as on the device
        return self.order[m0:n], cw / cw[-1]

    def sample(self, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0, u=None, c=None) -> int:
        if self.greedy_case(temperature, top_p, top_k):
            return S.greedy(self.l64)
        if not self.finite:
            return 0
        toks, cum = self.candidates(temperature, top_p, top_k, min_p, cut, seed, step, c)
        u = S.uniform(seed, step) if u is None else u
        r = int(np.searchsorted(cum, u, side="left"))      # the first rank with u <= cum[r]
        return int(toks[r] if r < toks.size else toks[0])

    # ---- ambiguity
    def ambiguous(self, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0) -> bool:
        if self.greedy_case(temperature, top_p, top_k) or not self.finite:
            return False
        cut = normal(cut)
        n_p, n_k, n_m = self.counts(top_p, top_k, min_p)
        n_s, n_e, n_h = self.cut_counts(cut)
        counts = {"p": n_p, "k": n_k, "m": n_m, "s": n_s, "e": n_e, "h": n_h}

        def reach(own):     # the ranks at which this cut can still change n: those no other cut has dropped, and one more
            return min(min(v for k, v in counts.items() if k != own) + 1, self.V)
        if top_p < 1.0 and np.any(np.abs(self.before[:reach("p")] - top_p) < S.PREFIX_SLACK):
            return True
        # a -inf logit (p = 0, d = -inf) is on the far side of every finite threshold: never near one
        ad, lnS, near = np.where(np.isfinite(self.d), np.abs(self.d), 0.0), abs(self.lnS), np.isfinite(self.d)
        with np.errstate(invalid="ignore"):
            if cut.top_n_sigma > 0.0:
                r = reach("s")
                bound = cut.top_n_sigma * (self.span * 2.0 ** -20 + 2.0 ** -22 * self.sigma) + 2.0 ** -23 * ad[:r]
                if np.any((np.abs(-self.d[:r] - cut.top_n_sigma * self.sigma) <= bound)[1:] & near[1:r]):
                    return True
            if cut.epsilon > 0.0:
                r = reach("e")
                bound = LN_S_ERR + 2.0 ** -22 * (ad[:r] + abs(ln(cut.epsilon)) + lnS)
                if np.any((np.abs(self.lnp[:r] - ln(cut.epsilon)) <= bound)[1:] & near[1:r]):
                    return True
            if cut.eta > 0.0:
                r = reach("h")
                bound = 2 * LN_S_ERR + 2.0 ** -21 * (1.0 + ad[:r] + abs(ln(cut.eta)) + self.H + lnS)
                if np.any((np.abs(self.lnp[:r] - self.eta_ln(cut.eta)) <= bound)[1:] & near[1:r]):
                    return True
            if cut.xtc_p > 0.0:
                c = coin(seed, step)
                if abs(c - cut.xtc_p) <= float(np.spacing(np.float32(cut.xtc_p))):
                    return True
                if c < cut.xtc_p:
                    r = min(min(counts.values()) + 1, self.V)
                    lt = ln(cut.xtc_t)
                    if lt > -np.inf:
                        bound = LN_S_ERR + 2.0 ** -22 * (ad[:r] + abs(lt) + lnS)
                        if np.any((np.abs(self.lnp[:r] - lt) <= bound) & near[:r]):
                            return True
        _, cum = self.candidates(temperature, top_p, top_k, min_p, cut, seed, step)
        u = S.uniform(seed, step)
        return bool(min(abs(u), np.min(np.abs(cum - u))) < S.EDGE_SLACK)


def sample(logits, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0, u=None, c=None) -> int:
    return Row(logits).sample(temperature, top_p, top_k, min_p, cut, seed, step, u, c)


def candidates(logits, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0, c=None):
    """(tokens of the candidate set in rank order, their normalised weights)."""
    toks, cum = Row(logits).candidates(temperature, top_p, top_k, min_p, cut, seed, step, c)
    return toks, np.diff(np.concatenate([[0.0], cum]))


# ----------------------------------------------------------------------------- the kernel's own arithmetic
def emulate(logits, temperature, top_p, top_k=0, min_p=0.0, cut=OFF, seed=0, step=0) -> int:
    """sample_rows_kernel<*, SAMPLE_CUT> restated operation by operation in f32 / integer arithmetic: the fixed-point moments, the
    integer sigma, the one lower bound on l - max, the count / min-key pass and the bounded integer draw.  (The boundary descent of top_p /
    top_k is the filtered kernel's: its result, the boundary rank, is taken in fixed point here as well.)"""
    f = np.float32
    l = F.clean32(logits)
    V = l.size
    cut = normal(cut)
    kcount = F.top_k_count(int(top_k), V)
    if temperature == 0.0 or top_p == 0.0 or not (l > -np.inf).any() or kcount == 1:
        return S.greedy(l.astype(np.float64))
    order = np.lexsort((np.arange(V), -l.astype(np.float64)))
    mx = l.max()
    fin = l > f(-np.inf)
    low = l[fin].min()
    ONE = f(2.0 ** 40)
    with np.errstate(all="ignore"):
        d = np.where(l == mx, f(0.0), (l - mx).astype(f)).astype(f)
        e = np.where(l == mx, f(1.0), np.exp(d)).astype(f)
    fx = lambda x: [int(v) for v in np.floor(x.astype(np.float64))]           # noqa: E731  (unsigned long long)(float)
    # the upper boundary of top_p / top_k in fixed point: the last rank whose mass before it is <= floor(P * total)
    mass = fx((e * ONE).astype(f))
    kmin_rank = V - 1
    if top_p < 1.0:
        total = sum(mass[i] for i in range(V))
        target = int(np.floor(np.float64(f(top_p)) * np.float64(total)))
        before, kmin_rank = 0, 0
        for r, i in enumerate(order):
            if before <= target:
                kmin_rank = r
            before += mass[i]
    kmin_rank = min(kmin_rank, kcount - 1)
    thr = F.ln_min_p(min_p)
    u_h, u_e, xtc = cut.eta > 0.0, cut.epsilon > 0.0, coin(seed, step) < cut.xtc_p
    thr_x = f(0.0)
    with np.errstate(all="ignore"):
        if u_h or u_e or xtc:
            g = np.where(l == mx, f(0.0), (mx - l).astype(f)).astype(f)
            eg = np.where(fin & (e > 0), (e * g).astype(f), f(0.0)).astype(f)
            se = sum(m for m, k in zip(mass, fin) if k)
            seg = sum(fx((eg * ONE).astype(f)))
            ln_s = f(f(np.log(f(se))) - f(27.725887222397812))
            if u_e:
                thr = max(thr, f(f(ln(cut.epsilon)) + ln_s))
            if u_h:
                h = f(ln_s + f(np.float64(seg) / np.float64(se)))
                le = f(ln(cut.eta))
                thr = max(thr, f(min(le, f(f(f(0.5) * le) - h)) + ln_s))
            thr_x = f(f(ln(cut.xtc_t)) + ln_s)
        qs = f(f(2097152.0) / f(mx - low))
        if cut.top_n_sigma > 0.0 and qs > 0 and qs < np.inf:
            q = [int(min(float(f(f(mx - x) * qs)), 2097152.0)) for x in l[fin]]
            cn, t1, t2 = len(q), sum(q), sum(v * v for v in q)
            sigma = f(np.sqrt(np.float64(cn * t2 - t1 * t1)) / (np.float64(cn) * np.float64(qs)))
            thr = max(thr, f(-f(f(cut.top_n_sigma) * sigma)))
    cand = [r for r, i in enumerate(order) if r <= kmin_rank and (r == 0 or d[i] >= thr)]
    mw = mx
    if xtc:
        over = [r for r in cand if d[order[r]] >= thr_x]
        if len(over) >= 2:
            cand = [r for r in cand if r >= over[-1]]
            mw = l[order[over[-1]]]
    inv_t = f(f(1.0) / f(temperature))
    with np.errstate(all="ignore"):
        w = [1 << 40 if l[order[r]] == mw else int(np.floor(np.float64(f(f(np.exp(f(f(l[order[r]] - mw) * inv_t))) * ONE)))) for r in cand]
    U = S.splitmix(seed, step) >> 40
    target = -((-U * sum(w)) >> 24)                        # ceil(U * W / 2^24)
    acc = 0
    for r, wi in zip(cand, w):
        acc += wi
        if acc >= target:
            return int(order[r])
    return int(order[0])
