"""Hand-worked cases of tests/cut_ref.py, the restatement the cut sampler (XTC, top-n-sigma, eta / epsilon cut-offs) is
held to; its identities; the mutants it must differ from on the grid of tests/cut_cases.py; the check that the grid leaves enough
unambiguous cases; the emulation of the kernel's own arithmetic; and the declarations of the ABI."""
import inspect
import math
import os
import re

import numpy as np
import pytest

import cut_cases as CC
import cut_ref as CR
import filter_ref as F
import sampling_ref as S
from cut_ref import Cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P5 = np.log(np.array([0.4, 0.3, 0.15, 0.1, 0.05]))
NINF = -np.inf


def ranks(l, cut=Cut(), top_p=1.0, top_k=0, min_p=0.0, c=0.0, T=1.0):
    """The candidate tokens, in rank order, of a row whose coin is c."""
    return CR.Row(l).candidates(T, top_p, top_k, min_p, cut, c=c)[0].tolist()


# ----------------------------------------------------------------------------- 1. each cut alone
def test_top_n_sigma_counts_the_logits_within_n_population_deviations_of_the_maximum():
    l = [4.0, 3.0, 2.0, 1.0, 0.0]                   # population sigma = sqrt(2)
    assert CR.Row(l).sigma == pytest.approx(math.sqrt(2.0))
    assert ranks(l, Cut(top_n_sigma=1.0)) == [0, 1]             # l >= 4 - 1.414
    assert ranks(l, Cut(top_n_sigma=1.5)) == [0, 1, 2]          # l >= 1.879
    assert ranks(l, Cut(top_n_sigma=0.5)) == [0]
    assert ranks(l, Cut(top_n_sigma=0.0)) == [0, 1, 2, 3, 4]    # off
    assert ranks(l, Cut(top_n_sigma=np.inf)) == [0, 1, 2, 3, 4]
    # -inf logits are not part of sigma
    assert CR.Row([4.0, NINF, 2.0, NINF, 0.0]).sigma == pytest.approx(float(np.std([4.0, 2.0, 0.0])))
    # the draw is inside the survivors with weights p^(1/T)
    toks, w = CR.candidates(l, 2.0, 1.0, cut=Cut(top_n_sigma=1.0))
    e = np.exp(np.array([0.0, -1.0]) / 2.0)
    assert toks.tolist() == [0, 1] and np.allclose(w, e / e.sum())


def test_epsilon_cutoff_keeps_p_at_least_epsilon_and_rank_0():
    assert ranks(P5, Cut(epsilon=0.12)) == [0, 1, 2]
    assert ranks(P5, Cut(epsilon=0.04)) == [0, 1, 2, 3, 4]
    assert ranks(P5, Cut(epsilon=0.5)) == [0]                   # nothing reaches it: rank 0 stays
    assert ranks([1.0, 1.0, 0.0], Cut(epsilon=0.9)) == [0]      # ... rank 0 alone, not the ties of the maximum
    assert ranks(P5, Cut(epsilon=0.0)) == [0, 1, 2, 3, 4]


def test_eta_cutoff_is_the_smaller_of_eta_and_its_entropy_scaled_root():
    r = CR.Row(P5)
    H = -sum(p * math.log(p) for p in (0.4, 0.3, 0.15, 0.1, 0.05))
    assert r.H == pytest.approx(H) and math.exp(-H) == pytest.approx(0.2485, abs=1e-4)
    assert ranks(P5, Cut(eta=0.2)) == [0, 1, 2]                 # min(0.2, 0.4472 * 0.2485 = 0.111): 0.15 stays, 0.1 goes
    assert ranks(P5, Cut(eta=0.09)) == [0, 1, 2, 3]             # min(0.09, 0.3 * 0.2485 = 0.0746): eta's root side binds
    assert ranks(P5, Cut(eta=0.004)) == [0, 1, 2, 3, 4]         # min(0.004, 0.0157): eta itself
    assert ranks(P5, Cut(eta=1.0)) == [0, 1]                    # min(1, exp(-H) = 0.2485)
    # a -inf logit adds nothing to H
    assert CR.Row(np.concatenate([P5, [NINF, NINF]])).H == pytest.approx(H)


# ----------------------------------------------------------------------------- 2. XTC
def test_xtc_with_m_0_1_2_and_V():
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.45)) == [0, 1, 2, 3, 4]     # m = 0
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.35)) == [0, 1, 2, 3, 4]     # m = 1: nothing to exclude
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.25)) == [1, 2, 3, 4]        # m = 2: the top goes, the least likely of the two stays
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.12)) == [2, 3, 4]           # m = 3
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.0)) == [4]                  # m = V: the least likely token alone
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.6)) == [0, 1, 2, 3, 4]      # a threshold above one half is off
    assert ranks(P5, Cut(xtc_p=0.0, xtc_t=0.12)) == [0, 1, 2, 3, 4]
    # the coin decides: c < probability excludes, c >= probability does not
    assert ranks(P5, Cut(xtc_p=0.5, xtc_t=0.12), c=0.49) == [2, 3, 4]
    assert ranks(P5, Cut(xtc_p=0.5, xtc_t=0.12), c=0.5) == [0, 1, 2, 3, 4]
    # the draw runs over the survivors alone: u against (0.15, 0.1, 0.05) / 0.3
    r = CR.Row(P5)
    cut = Cut(xtc_p=1.0, xtc_t=0.12)
    assert [r.sample(1.0, 1.0, cut=cut, u=u, c=0.0) for u in (0.0, 0.49, 0.51, 0.84, 0.99)] == [2, 2, 3, 4, 4]
    toks, w = CR.candidates(P5, 0.5, 1.0, cut=cut, c=0.0)
    assert np.allclose(w, np.array([0.15, 0.1, 0.05]) ** 2 / (np.array([0.15, 0.1, 0.05]) ** 2).sum())


def test_xtc_where_the_other_cuts_leave_fewer_than_m_ranks():
    cut = Cut(xtc_p=1.0, xtc_t=0.08)                                    # m = 4
    assert ranks(P5, cut) == [3, 4]
    assert ranks(P5, cut, top_k=2) == [1]                               # n = 2: m' = 2, the boundary rank stays
    assert ranks(P5, cut, top_k=3) == [2]
    assert ranks(P5, cut, min_p=0.5) == [1]                             # n_M = 2: 0.3 / 0.4 >= 0.5 > 0.15 / 0.4
    assert ranks(P5, cut, top_p=0.5) == [1]                             # n_P = 2: before = 0, 0.4, 0.7
    assert ranks(P5, Cut(epsilon=0.12, xtc_p=1.0, xtc_t=0.08)) == [2]   # n_E = 3
    assert ranks(P5, cut, top_k=5, min_p=0.2) == [3]                    # n_M = 4 = m: rank 3 alone
    # the probabilities are the whole row's: with top_k = 2 the survivors' renormalised 0.571 / 0.429 would both pass 0.41, the row's do not
    assert ranks(P5, Cut(xtc_p=1.0, xtc_t=0.41), top_k=2) == [0, 1]
    # the set is never empty
    for k in (1, 2, 3, 4, 5):
        for t in (0.0, 0.04, 0.2, 0.5):
            assert len(ranks(P5, Cut(xtc_p=1.0, xtc_t=t), top_k=max(k, 2))) >= 1


def test_xtc_ties_at_the_threshold():
    l = [2.0, 2.0, 1.0, 1.0, 0.0]                   # p = .307 .307 .113 .113 .042
    assert ranks(l, Cut(xtc_p=1.0, xtc_t=0.1)) == [3, 4]                # both tied tokens are over: the one of the higher index stays
    assert ranks(l, Cut(xtc_p=1.0, xtc_t=0.2)) == [1, 2, 3, 4]
    # p == threshold exactly counts as over: two tokens of one half each
    assert math.log(0.5) == -math.log(2.0)
    assert ranks([0.0, 0.0], Cut(xtc_p=1.0, xtc_t=0.5)) == [1]


def test_degenerate_rows():
    one = [NINF, 3.0, NINF]                          # one finite logit: sigma = 0, p = (1, 0, 0)
    r = CR.Row(one)
    assert r.sigma == 0.0 and r.H == 0.0
    assert ranks(one, Cut(top_n_sigma=2.0)) == [1]
    assert ranks(one, Cut(epsilon=0.5)) == [1] and ranks(one, Cut(eta=0.5)) == [1]
    assert ranks(one, Cut(xtc_p=1.0, xtc_t=0.3)) == [1, 0, 2]           # m = 1
    assert ranks(one, Cut(xtc_p=1.0, xtc_t=0.0)) == [2]                 # m = V: p >= 0 holds for the -inf tokens too
    assert CR.sample(one, 1.0, 1.0, cut=Cut(xtc_p=1.0, xtc_t=0.0), u=0.3, c=0.0) == 2
    for cut in (Cut(top_n_sigma=1.0), Cut(epsilon=0.1), Cut(eta=0.1), Cut(xtc_p=1.0, xtc_t=0.1)):
        assert CR.sample([NINF, np.nan, NINF], 1.0, 0.9, cut=cut) == 0  # an all -inf row: the greedy answer 0
        assert CR.sample([7.0], 1.0, 1.0, cut=cut, seed=3) == 0         # V = 1
    ties = [np.inf, 1.0, np.inf, 0.0]               # +inf ties: p = (.5, 0, .5, 0); sigma = 0 with a +inf in the row
    assert CR.Row(ties).sigma == 0.0
    assert ranks(ties, Cut(top_n_sigma=3.0)) == [0, 2]
    assert ranks(ties, Cut(epsilon=0.6)) == [0] and ranks(ties, Cut(epsilon=0.5)) == [0, 2]
    assert ranks(ties, Cut(xtc_p=1.0, xtc_t=0.5)) == [2, 1, 3]
    assert CR.sample(ties, 1.0, 1.0, cut=Cut(xtc_p=1.0, xtc_t=0.5), u=0.9, c=0.0) == 2
    # two equal finite logits: sigma = 0 keeps the ties of the maximum
    assert ranks([1.0, 1.0, NINF], Cut(top_n_sigma=1.0)) == [0, 1]


def test_the_coin_is_the_second_output_of_the_stream_that_gives_u():
    G = 0x9E3779B97F4A7C15
    for seed, step in ((0, 0), (1, 5), (0xFFFFFFFF, 0xFFFFFFFF), (77, 3)):
        state = ((seed << 32) | step) & S._MASK
        # SplitMix64 as published: state += G; output = mix(state).  sampling_ref.splitmix(seed, step) is the first output ...
        first = S.splitmix(seed, step)
        # ... and the second is the first output of the generator started one increment later
        s1 = (state + G) & S._MASK
        second = S.splitmix(s1 >> 32, s1 & 0xFFFFFFFF)
        assert CR.coin(seed, step) == float(second >> 40) * 2.0 ** -24
        assert first != second and 0.0 <= CR.coin(seed, step) < 1.0


# ----------------------------------------------------------------------------- 3. identities
def test_everything_off_is_filter_ref_and_threshold_above_half_is_off():
    rng = np.random.default_rng(5)
    offs = (Cut(), Cut(xtc_p=1.0, xtc_t=0.51), Cut(xtc_p=0.0, xtc_t=0.1), Cut(top_n_sigma=0.0, epsilon=0.0, eta=0.0))
    for V in (1, 7, 300):
        l = rng.normal(0, 2, V).astype(np.float32)
        l[rng.random(V) < 0.2] = NINF
        l[0] = 1.0
        row, frow = CR.Row(l), F.Row(l)
        for T, P, K, M in ((0.7, 0.3, 0, 0.0), (1.0, 0.9, 5, 0.1), (1.5, 1.0, 0, 0.0), (0.0, 0.5, 0, 0.0), (1.0, 0.0, 3, 0.0)):
            for seed in range(12):
                want = frow.sample(T, P, K, M, seed, 2)
                for cut in offs:
                    assert CR.is_off(cut)
                    assert row.sample(T, P, K, M, cut, seed, 2) == want
                    assert row.ambiguous(T, P, K, M, cut, seed, 2) == frow.ambiguous(T, P, K, M, seed, 2)


def test_top_k_one_and_temperature_zero_are_the_argmax():
    l = np.array([0.5, 2.0, 2.0, -1.0], np.float32)
    cut = Cut(2.0, 0.01, 0.01, 1.0, 0.1)
    assert CR.sample(l, 0.8, 0.9, top_k=1, cut=cut, u=0.99) == 1        # XTC would have removed token 1: no cut applies
    assert CR.sample(l, 0.0, 0.9, cut=cut) == 1 and CR.sample(l, 1.0, 0.0, cut=cut) == 1
    assert CR.sample([-3.2e38, -3.3e38], 1.0, 1.0, top_k=1, cut=cut) == 0
    assert not CR.Row(l).ambiguous(0.8, 0.9, top_k=1, cut=cut)


# ----------------------------------------------------------------------------- 4. mutants
class RemovesAll(CR.Row):               # XTC that removes all m (keeping the set non-empty)
    def xtc_first(self, m):
        return min(m, self._n - 1)

    def span_of(self, temperature, top_p, top_k=0, min_p=0.0, cut=CR.OFF, seed=0, step=0, c=None):
        self._n = self.upper(top_p, top_k, min_p, CR.normal(cut))
        return super().span_of(temperature, top_p, top_k, min_p, cut, seed, step, c)


class Renormalised(CR.Row):             # XTC on the probabilities renormalised over the n survivors, as llama.cpp has them
    def xtc_count(self, cut, n):
        with np.errstate(all="ignore"):
            p = np.exp(self.lnp[:n])
            return int(np.count_nonzero(p / p.sum() >= CR.normal(cut).xtc_t))


class SampleDeviation(CR.Row):
    def sigma_of(self):
        return self.sample_sigma


class EtaWithoutMin(CR.Row):
    def eta_ln(self, eta):
        return 0.5 * CR.ln(eta) - self.H


class CoinIsU(CR.Row):
    def coin_of(self, seed, step):
        return S.uniform(seed, step)


@pytest.mark.parametrize("mutant", [RemovesAll, Renormalised, SampleDeviation, EtaWithoutMin, CoinIsU])
def test_the_reference_differs_from_the_mutant_on_the_grid(mutant):
    differ = 0
    for V in (2, 50, 1000):         # V = 2: where the sample deviation is sqrt(2) times the population one
        for name, l, g, want in CC.expected(V):
            mrow = mutant(l)
            differ += sum(w is not None and mrow.sample(t, p, k, m, c, s, CC.STEP) != w for (t, p, k, m, c, s), w in zip(g, want))
    assert differ >= 1, (mutant.__name__, differ)


# ----------------------------------------------------------------------------- 5. the grid and the kernel's arithmetic
@pytest.mark.parametrize("V", CC.VOCABS)
def test_the_gpu_rows_leave_95_percent_of_the_cases_clear(V):
    for _, _, g, _ in CC.expected(V):
        assert len(g) == len(CC.CUTS) * len(CC.FILTERS) * len(CC.TEMPS) * len(CC.SEEDS)
    total = sum(len(w) for _, _, _, w in CC.expected(V))
    clear = sum(x is not None for _, _, _, w in CC.expected(V) for x in w)
    assert clear >= 0.95 * total, (V, clear, total)


def test_the_grid_exercises_every_cut():
    """Each cut binds (changes the candidate set) in a good share of its cases, XTC both ways of the coin."""
    row = CR.Row(CC.rows_for(1000)[1][1])
    bound = {"s": 0, "e": 0, "h": 0, "x": 0, "coin_up": 0}
    for t, p, k, m, c, s in CC.grid(1000):
        if row.greedy_case(t, p, k):
            continue
        n_f = min(row.counts(p, k, m))
        n_s, n_e, n_h = row.cut_counts(c)
        bound["s"] += n_s < n_f
        bound["e"] += n_e < n_f
        bound["h"] += n_h < n_f
        m0, _ = row.span_of(t, p, k, m, c, s, CC.STEP)
        bound["x"] += m0 > 0
        bound["coin_up"] += CR.normal(c).xtc_p > 0 and CR.coin(s, CC.STEP) >= CR.normal(c).xtc_p
    assert all(v >= 5 for v in bound.values()), bound


@pytest.mark.parametrize("V,every", [(1, 1), (50, 1), (1000, 3)])
def test_the_emulation_of_the_kernels_arithmetic_agrees_on_the_clear_cases(V, every):
    checked = 0
    for name, l, g, want in CC.expected(V):
        for (t, p, k, m, c, s), w in list(zip(g, want))[::every]:
            if w is None:
                continue
            assert CR.emulate(l, t, p, k, m, c, s, CC.STEP) == w, (name, (t, p, k, m, c, s))
            checked += 1
    assert checked >= 0.9 * sum(len(g[::every]) for _, _, g, _ in CC.expected(V))


def test_the_bounds_are_what_the_docstring_derives():
    assert CR.LN_S_ERR == 2.0 ** -16 and 2.0 ** -22 + 2.0 ** -20 + 2.0 ** -18 + 2.0 ** -18 < CR.LN_S_ERR
    # a token exactly at a threshold is ambiguous, one a thousand bounds away is not
    r = CR.Row(P5)
    assert r.ambiguous(1.0, 1.0, cut=Cut(epsilon=math.exp(r.lnp[2])), seed=1)
    assert r.ambiguous(1.0, 1.0, cut=Cut(top_n_sigma=float(-r.d[3] / r.sigma)), seed=1)
    assert not r.ambiguous(1.0, 1.0, cut=Cut(epsilon=0.12, top_n_sigma=1.3), seed=1) or \
        abs(S.uniform(1, 0) - 0.5) < 0.5            # (the draw may still sit on an edge: only the cut bounds are under test)
    # a rank another cut has dropped excuses nothing
    assert not r.ambiguous(1.0, 1.0, top_k=2, cut=Cut(epsilon=math.exp(r.lnp[4])), seed=1) or \
        r.ambiguous(1.0, 1.0, top_k=2, seed=1)


# ----------------------------------------------------------------------------- 6. the ABI
def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wrk_hip.h")).read(), flags=re.S)


def fields(cname):
    body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", header(), flags=re.S).group(1)
    return [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]


FIVE = ["top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc_probability", "xtc_threshold"]


def test_cut_entry_points_are_declared_exported_and_bound():
    import wrk
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", header()))
    for name, nargs in (("wrk_sample_logits_cut", 17), ("wrk_v7_generate_queue_cut", 9), ("wrk_v6_generate_queue_cut", 9)):
        assert name in declared and hasattr(wrk.hip, name) and name in wrk.HIP_SYMBOLS
        assert len(wrk.HIP_SYMBOLS[name][1]) == nargs
    names = fields("wrk_generate_options")
    assert names == [n for n, _ in wrk.GenerateOptions._fields_]
    at = names.index("poll_steps")
    assert names[at + 1:at + 6] == FIVE and names[at + 6] == "num_top" and names[-2:] == ["top_k", "min_p"]
    assert all(not getattr(wrk.GenerateOptions(), n) for n in FIVE)         # NULL in a zeroed struct: off
    # the queue's options keep their fields: the arrays travel beside them
    assert not set(FIVE) & set(fields("wrk_queue_options"))
    assert fields("wrk_queue_cuts") == FIVE + ["pool", "guide"] == [n for n, _ in wrk.QueueCuts._fields_]


def test_python_entry_points_take_the_four_keywords():
    import wrk
    for fn in (wrk.Context.sample_logits, wrk.Runtime.generate_sample, wrk.Runtime.generate_penalized, wrk.Runtime.generate_stop,
               wrk.Runtime.generate_guided, wrk.Runtime.generate_queue, wrk.Runtime.generate_queue_guided):
        par = inspect.signature(fn).parameters
        for name in ("top_n_sigma", "epsilon_cutoff", "eta_cutoff", "xtc"):
            assert name in par and par[name].default is None, (fn.__name__, name)
