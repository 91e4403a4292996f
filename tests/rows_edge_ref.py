"""What the logits-row kernels are to give on the rows of tests/rows_edge_cases.py.  Not a test module: tests/test_rows_edge_ref.py
checks it on the CPU, tests/test_gpu_rows_edges.py holds the kernels to it.

canonical(row): the row as the sampler family is specified to read it -- NaN becomes -inf; if any +inf is present, every +inf becomes
0.0 and everything else -inf (the limit of softmax as the top logits grow, and what the kernel's `l == mx` guards compute).  The kernels
get the raw row; sampling_ref, filter_ref.Row, mirostat_ref.Row and typical_ref.Row get the canonical one.

Exact weights.  The kernel's masses are floor(e * 2^40) with e = 1 where l == mx and expf(x) elsewhere, x = fl(fl(l - mx) * fl(1 / T))
(the nucleus: T = 1).  Where every x is either at most 2^-26 in magnitude (expf rounds to exactly 1.0f: 1 - 2^-26 lies within half an
ulp of 1) or below -30 (e < 2^-43: the mass truncates to 0), the masses are exactly 2^40 or 0, every sum is an exact integer and the
drawn token follows in integers from the kernel's header comment and sampling_ref:
  * the m weight-1 tokens are a prefix of the sampler's order (logit descending, index ascending);
  * U = splitmix(seed, step) >> 40;
  * nucleus: "the last rank whose mass before it is <= P * sum": rank r is in iff r * 2^40 <= floor(P64 * m * 2^40), P64 the f32 top_p
    widened to double (the product is exact: 24 + 20 + 40 bits), iff r <= floor(P64 * m): n = min(m, floor(P64 * m) + 1); P >= 1: n = m;
  * top-k: min(n, k); min-p: the exact f32 count of filter_ref.min_p_count (it drops weight-1 tokens only on the subnormal rows at
    min_p = 1); typical, where the weight-1 tokens share one value: g = 0 on them, gbar = 0, d = 0, so the typical order is the
    sampler's among them and its cut is the nucleus formula with typical_p (the subnormal rows are left out of this mode: their d
    differ at the 1e-39 scale, far inside the rounding of gbar, so no order among them is specified); Mirostat: W = m, every weight-1 token has surprise log2 m: all m are candidates if log2 m <= mu, else rank 0 alone;
  * draw: "the first rank whose mass up to and including it is >= ceil(U * W / 2^24)", W = c * 2^40: rank max(ceil(U * c / 2^24) - 1, 0).
Where the draw's weights are exact but the nucleus masses (T = 1) are not -- a spread row at T <= 1e-30 or T = 3e38 -- the nucleus count
comes from the f64 reference at P -+ PREFIX_SLACK and the case is ambiguous only if the two counts draw different tokens (the drawn
rank is monotone in the count).
"""
import functools
import math

import numpy as np

import alt_cases as AC
import filter_cases as FC
import filter_ref as F
import logprob_ref as L
import mirostat_ref as M
import rows_edge_cases as RC
import sampling_ref as S
import score_ref as SC
import typical_ref as TY

STEP = 5
MUTANTS = ("nan_pos_inf", "tie_high_index", "inf_ties_first", "neg_zero_below")


# ----------------------------------------------------------------------------- the row as the sampler reads it
def canonical(row, mutant=None) -> np.ndarray:
    l = np.array(row, np.float32)
    nan = np.isnan(l)
    l[nan] = np.inf if mutant == "nan_pos_inf" else -np.inf
    top = l == np.inf
    if top.any():
        if mutant == "inf_ties_first":
            top[np.flatnonzero(top)[1:]] = False
        l = np.where(top, np.float32(0.0), np.float32(-np.inf)).astype(np.float32)
    return l


def order_of(l, mutant=None) -> np.ndarray:
    """The sampler's order of a canonical row: logit descending (-0 == +0), ties by index ascending."""
    v = np.asarray(l, np.float64) + 0.0
    if mutant == "neg_zero_below":
        v = np.where((v == 0.0) & np.signbit(np.asarray(l)), -1e-300, v)
    idx = np.arange(v.size)
    return np.lexsort((-idx if mutant == "tie_high_index" else idx, -v))


def greedy(row, mutant=None) -> int:
    """argmax_rows: the first index of the maximum after row_norm, 0 when nothing exceeds -3e38 (+inf is not taken to the limit here:
    the maximum of the raw row)."""
    l = np.array(row, np.float32)
    l[np.isnan(l)] = np.inf if mutant == "nan_pos_inf" else -np.inf
    if not (l > np.float32(-3.0e38)).any():
        return 0
    o = order_of(l, mutant)
    return int(o[0])


# ----------------------------------------------------------------------------- exact weights
def _x32(l, temperature):
    """fl(fl(l - mx) * fl(1 / T)) off the maximum, 0 on it, as the kernel evaluates it."""
    f = np.float32
    mx = l.max()
    with np.errstate(all="ignore"):
        inv_t = f(1.0) / f(temperature)
        x = ((l - mx).astype(f) * inv_t).astype(f)
    return np.where(l == mx, f(0.0), x)


def weight_one(l, temperature):
    """Boolean mask of the weight-1 tokens of a canonical row at `temperature`, or None where some weight is neither exactly 1 nor 0."""
    x = _x32(l, temperature)
    one = np.abs(x) <= 2.0 ** -26
    zero = x < -30.0
    return one if bool(np.all(one | zero)) else None


class Exact:
    """A canonical row whose draw weights at `temperature` are exactly 0 or 1."""

    def __init__(self, row, temperature, mutant=None):
        self.l = canonical(row, mutant)
        self.V = self.l.size
        assert (self.l > -np.inf).any()
        self.order = order_of(self.l, mutant)
        one_t = weight_one(self.l, temperature)
        assert one_t is not None, "not an exact-weight row at this temperature"
        self.m_t = int(one_t.sum())
        assert one_t[self.order[:self.m_t]].all()           # a prefix of the order
        one_1 = weight_one(self.l, 1.0)
        self.m_1 = None if one_1 is None else int(one_1.sum())
        self.one_value = bool(np.unique(self.l[self.order[:self.m_t]] + np.float32(0.0)).size == 1)
        self._before = None

    def nucleus(self, top_p):
        """(count at the low end of the slack, count at the high end); equal where the T = 1 masses are exact."""
        p = float(np.float32(top_p))
        if p >= 1.0:
            return self.V, self.V
        if self.m_1 is not None:
            n = min(self.m_1, int(math.floor(p * self.m_1)) + 1)
            return n, n
        if self._before is None:
            self._before = S.nucleus(self.l.astype(np.float64), 1.0, 1.0)[2]
        lo = max(1, int(np.count_nonzero(self._before <= p - S.PREFIX_SLACK)))
        return lo, max(1, int(np.count_nonzero(self._before <= p + S.PREFIX_SLACK)))

    def pick(self, count, seed, step=STEP):
        U = S.splitmix(seed, step) >> 40
        return int(self.order[max(-((-U * count) >> 24) - 1, 0)])

    def sample(self, top_p, seed, step=STEP, top_k=0, min_p=0.0, typical_p=1.0):
        """The drawn token, or None where the nucleus count is ambiguous and matters."""
        if float(np.float32(typical_p)) < 1.0:
            assert self.m_1 is not None and self.one_value, "the typical order is exact only among equal logits"
            tp = float(np.float32(typical_p))
            lo = hi = min(self.m_1, int(math.floor(tp * self.m_1)) + 1)
        else:
            lo, hi = self.nucleus(top_p)
        cap = min(self.m_t, F.top_k_count(top_k, self.V), F.min_p_count(self.l, min_p))
        a, b = self.pick(min(lo, cap), seed, step), self.pick(min(hi, cap), seed, step)
        return a if a == b else None

    def mirostat(self, mu, tau, eta, seed, step=STEP):
        """(token, mu after the draw, tolerance)"""
        lw = math.log2(self.m_t)
        assert abs(lw - mu) > 1e-3 or self.m_t == 1, "mu sits on the threshold"
        c = self.m_t if lw <= mu else 1
        s = math.log2(c)
        mu2 = mu - eta * (s - tau)
        return self.pick(c, seed, step), mu2, M.mu_tol(eta, tau, mu2, s, s, self.V)


# ----------------------------------------------------------------------------- seeds at the ends of u
def search_seeds(step=STEP, limit=1 << 27, chunk=1 << 22):
    """The first seeds whose U = splitmix(seed, step) >> 40 is 0 and 2^24 - 1 (vectorised; wraps modulo 2^64 as the kernel does)."""
    found = {}
    with np.errstate(over="ignore"):
        for a in range(0, limit, chunk):
            z = ((np.arange(a, a + chunk, dtype=np.uint64) << np.uint64(32)) | np.uint64(step)) + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            U = (z ^ (z >> np.uint64(31))) >> np.uint64(40)
            for want in (0, (1 << 24) - 1):
                hit = np.flatnonzero(U == np.uint64(want))
                if want not in found and hit.size:
                    found[want] = a + int(hit[0])
            if len(found) == 2:
                break
    return found.get(0), found.get((1 << 24) - 1)


SEED_U_ZERO, SEED_U_MAX = 4789276, 10276771         # search_seeds(STEP): u = 0 and u = 1 - 2^-24 at step 5


# ----------------------------------------------------------------------------- the cases of every sampler mode
def plain_grid(V):
    """tests/test_gpu_sampling.py's grid: P = 1.0 only with T <= 0.5 above V = 1000."""
    Ts = (0.1, 0.5, 1.0, 2.0)
    if V <= 1000:
        return [(T, P) for T in Ts for P in (0.05, 0.33, 0.71, 0.9, 1.0)]
    return [(T, P) for T in Ts for P in (0.05, 0.3, 0.7, 0.95)] + [(T, 1.0) for T in (0.1, 0.5)]


EXACT_TS = (0.1, 1.0, 2.0)
EXACT_PS = (0.05, 0.5, float(np.float32(1.0 - 2.0 ** -24)), 1.0)
EXACT_MUS = (0.5, 2.0, 5.0, 10.5, 20.0)         # clear of log2 m for every m these rows have (asserted)


def _seeds(k, salt):
    """two ordinary seeds per point, and on the exact rows the two ends of u"""
    return (1 + 16 * (k + salt), 7 + 16 * (k + salt))


def _salt(name, V):
    return 1000 * sorted(RC.PROFILES).index(name) + V


def filter_grid(V):
    """every fifth case of filter_cases.grid: 5 is coprime to the grid's inner sizes, so every top_ks(V) edge value still meets every
    min_p, top_p and temperature"""
    return FC.grid(V)[::5]


@functools.lru_cache(maxsize=None)
def plain_cases(name, V, mutant=None):
    """(raw row, [(T, P, seed)], [token, or None where the case is ambiguous])"""
    raw = RC.row(name, V)
    cases, want = [], []
    if name in RC.EXACT:
        for T in EXACT_TS:
            ex = Exact(raw, T, mutant)
            for P in EXACT_PS:
                for s in _seeds(len(cases), _salt(name, V)) + (SEED_U_ZERO, SEED_U_MAX):
                    cases.append((T, P, s))
                    want.append(ex.sample(P, s))
        assert None not in want
        return raw, cases, want
    l = canonical(raw, mutant).astype(np.float64)
    for T, P in plain_grid(V):
        for s in _seeds(len(cases), _salt(name, V)):
            cases.append((T, P, s))
            want.append(None if S.ambiguous(l, T, P, s, STEP) else S.sample(l, T, P, s, STEP))
    return raw, cases, want


@functools.lru_cache(maxsize=None)
def filter_cases(name, V):
    """(raw row, [(T, P, top_k, min_p, seed)], [token or None])"""
    raw = RC.row(name, V)
    g = filter_grid(V)
    if name in RC.EXACT:
        ex = {T: Exact(raw, T) for T in FC.TEMPS}
        want = []
        for T, P, K, mp, s in g:
            if T == 0.0 or P == 0.0 or F.top_k_count(K, V) == 1:
                want.append(greedy(raw))
            else:
                want.append(ex[T].sample(P, s, top_k=K, min_p=mp))
        assert None not in want
        return raw, g, want
    r = F.Row(canonical(raw))
    return raw, g, [None if r.ambiguous(T, P, K, mp, s, STEP) else r.sample(T, P, K, mp, s, STEP) for T, P, K, mp, s in g]


@functools.lru_cache(maxsize=None)
def mirostat_cases(name, V):
    """(raw row, [(T, mu, seed)], [(token, mu after, tolerance) or None]) at alt_cases' TAU and ETA"""
    raw = RC.row(name, V)
    if name in RC.EXACT:
        g = [(T, mu, s) for T, mu, s in AC.grid(EXACT_MUS, salt=_salt(name, V))]
        ex = {T: Exact(raw, T) for T in AC.TEMPS}
        return raw, g, [ex[T].mirostat(mu, AC.TAU, AC.ETA, s) for T, mu, s in g]
    g = AC.grid(AC.MUS, salt=_salt(name, V))
    rows = {T: M.Row(canonical(raw), T) for T in AC.TEMPS}
    want = []
    for T, mu, s in g:
        if rows[T].ambiguous(mu, s, STEP):
            want.append(None)
            continue
        tok, mu2, info = rows[T].step(mu, AC.TAU, AC.ETA, s, STEP)
        want.append((tok, mu2, M.mu_tol(AC.ETA, AC.TAU, mu2, info[0], info[1], V)))
    return raw, g, want


@functools.lru_cache(maxsize=None)
def typical_cases(name, V):
    """(raw row, [(T, typical_p, seed)], [token or None]); top_p = alt_cases.TOP_P is read by the typical_p = 1 rows only"""
    raw = RC.row(name, V)
    g = AC.grid(AC.TYPICAL_PS, salt=_salt(name, V))
    if name in RC.EXACT:
        ex = {T: Exact(raw, T) for T in AC.TEMPS}
        want = [ex[T].sample(AC.TOP_P, s, typical_p=tp) for T, tp, s in g]
        assert None not in want
        return raw, g, want
    r = TY.Row(canonical(raw))
    return raw, g, [None if r.ambiguous(T, AC.TOP_P, tp, s, STEP) else r.sample(T, AC.TOP_P, tp, s, STEP) for T, tp, s in g]


# temperature and top-p edges
EDGE_TS = (1e-45, 1.2e-38, 1e-30, 1e-3, 1e3, 3e38)
EDGE_PS = (1e-45, 1e-30, float(np.float32(1.0 - 2.0 ** -24)), 1.0, 7.0, np.inf)
EDGE_PROFILES = ("peaked", "nan_mix", "pos_inf_ties")
EDGE_VOCABS = (2, 1025, 8193)


def _spread_case(l64, T, P, seed):
    """sampling_ref.sample with sampling_ref.ambiguous's rule read at the counts: the nucleus is ambiguous only where P -+ PREFIX_SLACK
    changes its count (rank 0 is in at any P > 0, so its mass before, 0, excuses nothing), the draw where u is within EDGE_SLACK of an edge."""
    toks, w, before = S.nucleus(l64, T, P)
    if P < 1.0 and np.count_nonzero(before[1:] <= P - S.PREFIX_SLACK) != np.count_nonzero(before[1:] <= P + S.PREFIX_SLACK):
        return None
    edges = np.concatenate([[0.0], np.cumsum(w)])
    if np.min(np.abs(edges - S.uniform(seed, STEP))) < S.EDGE_SLACK:
        return None
    return S.sample(l64, T, P, seed, STEP)


@functools.lru_cache(maxsize=None)
def edge_cases(name, V):
    """(raw row, [(T, P, seed)], [token or None]) over EDGE_TS x EDGE_PS: the closed form wherever the draw's weights are exact (every
    T <= 1e-30 -- asserted -- and 3e38), sampling_ref with its ambiguity rule elsewhere.  On a spread row the two P = 1 - 2^-24 points
    at T = 1e3 and 3e38 are ambiguous by construction (the row's last tokens sit inside PREFIX_SLACK and the draw is all but
    uniform): 4 of 72 cases.  `edge_cap` therefore asks for 95 % of the other 68; those 4 are still compared wherever they are clear."""
    raw = RC.row(name, V)
    l = canonical(raw)
    cases, want = [], []
    for T in EDGE_TS:
        t32 = float(np.float32(T))
        exact = weight_one(l, t32) is not None
        assert exact or T > 1e-30
        ex = Exact(raw, t32) if exact else None
        for P in EDGE_PS:
            for s in _seeds(len(cases), _salt(name, V)):
                cases.append((T, P, s))
                want.append(ex.sample(P, s) if ex else _spread_case(l.astype(np.float64), t32, float(np.float32(P)), s))
    return raw, cases, want


def edge_cap(cases, want):
    """(unambiguous, total) over the cases that are not ambiguous by construction"""
    counted = [w is not None for (T, P, s), w in zip(cases, want) if not (T >= 1e3 and 0.99 < P < 1.0)]
    return sum(counted), len(counted)


BIG_CASES = (("all_equal_zero", 1.0, 1.0, SEED_U_MAX), ("all_equal_zero", 1.0, 0.5, SEED_U_MAX), ("subnormal", 1.0, 1.0, 3),
             ("pos_inf_ties", 2.0, 0.05, 4), ("huge_span", 1.0, 1.0, SEED_U_ZERO), ("offset_pos", 0.5, 0.7, 6), ("nan_mix", 1.0, 0.3, 7),
             ("deep_tail", 2.0, 0.95, 8))


@functools.lru_cache(maxsize=None)
def big_cases():
    """[(name, T, P, seed, token)] at V = 2^20, SAMPLE_MAX_VOCAB: W reaches 2^60 on the constant row, whose u = 1 - 2^-24 draw is the
    last index (P = 1) and index 2^19 (P = 0.5)."""
    out = []
    for name, T, P, s in BIG_CASES:
        raw = RC.row(name, RC.BIG_V)
        if name in RC.EXACT:
            out.append((name, T, P, s, Exact(raw, T).sample(P, s)))
        else:
            out.append((name, T, P, s, _spread_case(canonical(raw).astype(np.float64), T, P, s)))
    return out


def compare(label, got, want, cap=0.95):
    """Token equality on every unambiguous case; at least `cap` of the cases unambiguous.  Returns the number compared."""
    clear = 0
    for i, w in enumerate(want):
        if w is None:
            continue
        clear += 1
        assert int(got[i]) == int(w), (label, i, int(got[i]), int(w))
    assert clear >= cap * len(want), (label, clear, len(want))
    return clear


# ----------------------------------------------------------------------------- score and log-probs
def targets_for(row):
    """Target tokens on: the maximum, a tied maximum (its last holder), a -inf, a NaN, the lowest finite value, the last index."""
    x = np.asarray(row, np.float32)
    V = x.size
    c = np.where(np.isnan(x), np.float32(-np.inf), x)
    out = [int(np.argmax(c)), int(np.flatnonzero(c == c.max())[-1])]
    for mask in (x == -np.inf, np.isnan(x)):
        hit = np.flatnonzero(mask)
        out.append(int(hit[len(hit) // 2]) if hit.size else V // 2)
    fin = np.where(np.isfinite(x), x, np.float32(np.inf))
    out.append(int(np.argmin(fin)))
    out.append(V - 1)
    return out


def score_expected(row, targets):
    """(log-probs as f32 -- the f64 value of score_ref rounded to f32 --, ranks); a +inf anywhere: NaN (inf - inf)."""
    x = np.asarray(row, np.float32)
    with np.errstate(all="ignore"):
        lp, rk = SC.score_rows(np.tile(x.astype(np.float64), (len(targets), 1)), targets)
        lp = lp.astype(np.float32)
    if (x == np.inf).any():
        lp[:] = np.nan
    return lp, rk


def top_expected(row, targets, n):
    """(log-probs f32 [len(targets)], top ids [n] or None where the row holds a NaN, top log-probs f32 [n])"""
    x = np.asarray(row, np.float32)
    with np.errstate(all="ignore"):
        lp0, ids, tlp = L.top_row(x.astype(np.float64), int(targets[0]), n)
        if np.isnan(x).any():
            return np.full(len(targets), np.nan, np.float32), None, np.full(n, np.nan, np.float32)
        lp = L.log_softmax(x.astype(np.float64))[np.asarray(targets)].astype(np.float32)
        tlp = tlp.astype(np.float32)
    if (x == np.inf).any():
        lp[:] = np.nan
        tlp[:] = np.nan
    return lp, ids, tlp


# ----------------------------------------------------------------------------- penalties
def penalize32(x, counts, flags, ap, af):
    """penalty_ref.penalize's three roundings written out (t = c * af; t = ap + t; x - t, no FMA), on raw bits: NaN stays NaN."""
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        t = (np.asarray(counts, f) * f(af)).astype(f)
        t = (f(ap) + t).astype(f)
        y = (x - t).astype(f)
    fl = np.asarray(flags).astype(np.uint32)
    out = np.where(fl & 1, y, x)
    return np.where(fl & 2, f(-np.inf), out).astype(f)
