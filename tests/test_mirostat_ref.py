"""tests/mirostat_ref.py against hand-worked cases, sampling_ref (off rows), an f32 restatement of the device's evaluation (inside the
bounds) and mutants of the contract (outside them); the kernel test's rows leave 95 % of its cases unambiguous."""
import os
import re

import numpy as np
import pytest

import alt_cases as AC
import mirostat_ref as M
import sampling_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2 = np.log(2.0)


def test_hand_worked_two_bit_row():
    # p = (1/2, 1/4, 1/8, 1/8) at T = 1: surprises 1, 2, 3, 3 bits
    l = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    row = M.Row(l, 1.0)
    assert np.allclose(row.s, [1, 2, 3, 3])
    assert [row.count(mu) for mu in (0.5, 1.5, 1.99, 2.01, 2.5, 3.01, 9.0)] == [1, 1, 1, 2, 2, 4, 4]
    # mu = 2.5: candidates {0, 1} with weights 2/3, 1/3; u = 0.5 draws token 0, observed surprise log2(3/2)
    tok, mu2, (s, lw) = row.step(2.5, 3.0, 0.5, u=0.5)
    assert tok == 0 and np.isclose(s, np.log2(1.5)) and np.isclose(mu2, 2.5 - 0.5 * (np.log2(1.5) - 3.0))
    tok, mu2, (s, _) = row.step(2.5, 3.0, 0.5, u=0.7)
    assert tok == 1 and np.isclose(s, np.log2(3.0)) and np.isclose(mu2, 2.5 - 0.5 * (np.log2(3.0) - 3.0))
    # mu below the top token's surprise: one candidate, s == 0 exactly, mu moves by eta * tau
    tok, mu2, (s, lw) = row.step(0.25, 3.0, 0.5, u=0.99)
    assert tok == 0 and s == 0.0 and lw == 0.0 and mu2 == 0.25 + 1.5


def test_temperature_enters_the_surprise():
    l = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    row = M.Row(l, 0.5)         # weights p^2: 16 : 4 : 1 : 1 of 22
    assert np.allclose(row.s, -np.log2(np.array([16, 4, 1, 1]) / 22.0))


def test_ties_and_the_top_token():
    l = np.array([1.0, 3.0, 3.0, -np.inf, np.nan])
    row = M.Row(l, 1.0)
    assert list(row.order[:2]) == [1, 2]
    assert row.count(-5.0) == 1 and row.step(-5.0, 1.0, 0.0, u=0.999)[0] == 1      # rank 0 only: the first index of the maximum
    assert row.count(row.s[0]) == 2                                                 # equal surprise: both in


def test_greedy_and_off_rows():
    rng = np.random.default_rng(0)
    l = rng.normal(0, 2, 50).astype(np.float32)
    assert M.sample(l, 0.0, 0.3, 5.0, 0.1, 7.0) == (S.greedy(l), 7.0)
    assert M.sample(np.full(5, -np.inf), 1.0, 0.3, 5.0, 0.1, 7.0) == (0, 7.0)
    for seed in range(20):
        assert M.sample(l, 0.8, 0.6, 0.0, 0.1, 7.0, seed, 3) == (S.sample(l, 0.8, 0.6, seed, 3), 7.0)
        assert M.ambiguous(l, 0.8, 0.6, 0.0, 7.0, seed, 3) == S.ambiguous(l, 0.8, 0.6, seed, 3)
    # top_p is not read by a Mirostat row
    assert M.sample(l, 0.8, 0.0, 5.0, 0.1, 7.0, 4, 3) == M.sample(l, 0.8, 1.0, 5.0, 0.1, 7.0, 4, 3)
    assert M.start_mu(5.0) == 10.0


def _cases(V):
    for name, l, g, want in AC.mirostat_expected(V):
        for (t, mu, s), w in zip(g, want):
            yield name, l, t, mu, s, w


@pytest.mark.parametrize("V", [1, 50, 1000, 3000])
def test_f32_restatement_lies_inside_the_bounds(V):
    n = 0
    for name, l, t, mu, s, w in _cases(V):
        if w is None:
            continue
        tok, mu2 = M.sample32(l, t, AC.TAU, AC.ETA, mu, s, AC.STEP)
        assert tok == w[0], (V, name, t, mu, s)
        assert abs(mu2 - w[1]) <= w[2], (V, name, t, mu, s, mu2, w)
        n += 1
    assert n


def test_mutants_lie_outside_the_bounds():
    hits = {"sign": 0, "norm": 0, "start": 0}
    total = 0
    for name, l, t, mu, s, w in _cases(1000):
        if w is None:
            continue
        total += 1
        for variant in ("sign", "norm"):
            _, mu2 = M.sample32(l, t, AC.TAU, AC.ETA, mu, s, AC.STEP, variant=variant)
            hits[variant] += abs(mu2 - w[1]) > w[2]
    assert hits["sign"] == total            # eta (s - tau) is never within 1e-5 of 0 on these rows
    assert hits["norm"] >= total // 2       # the candidates are a proper subset in most cases: log2 W != log2 W_c
    # a fresh sequence starts at 2 tau: from tau the first draw of a peaked row has fewer candidates
    l = np.log(np.array([0.3, 0.25, 0.2, 0.15, 0.1]))
    row = M.Row(l, 1.0)
    assert row.count(M.start_mu(1.5)) != row.count(1.5)


@pytest.mark.parametrize("V", AC.VOCABS)
def test_the_gpu_rows_leave_95_percent_of_the_cases_clear(V):
    want = [w for _, _, _, ws in AC.mirostat_expected(V) for w in ws]
    assert len(want) == 4 * len(AC.MUS) * len(AC.TEMPS) * len(AC.SEEDS)
    clear = sum(w is not None for w in want)
    assert clear >= 0.95 * len(want), (V, clear, len(want))


def test_the_slacks_are_the_derived_ones():
    assert M.mu_slack(20.0, 65536) < 1e-4 and M.mu_slack(20.0, 65536) > 6 * M.EPS * 36
    assert 1e-6 < M.mu_tol(0.1, 5.0, 10.0, 3.0, 1.0, 65536) < 1e-5


def test_entry_points_and_fields_are_declared_exported_and_bound():
    import ctypes as C
    import wrk
    text = open(os.path.join(ROOT, "include", "wrk_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(wrk_[a-z0-9_]+)\s*\(", text))
    for name, nargs in (("wrk_sample_logits_mirostat", 13), ("wrk_sample_logits_typical", 11)):
        assert name in declared and hasattr(wrk.hip, name) and len(wrk.HIP_SYMBOLS[name][1]) == nargs
    for cname, cls in (("wrk_generate_options", wrk.GenerateOptions), ("wrk_queue_options", wrk.QueueOptions)):
        body = re.search(r"typedef\s+struct\s+" + cname + r"\s*\{(.*?)\}", text, flags=re.S).group(1)
        names = [n for stmt in body.split(";") if stmt.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", stmt.strip())]
        assert names == [n for n, _ in cls._fields_], cname
        assert names[-6:] == ["mirostat_tau", "mirostat_eta", "mirostat_mu", "typical_p", "top_k", "min_p"]
        assert all(C.sizeof(t) == 8 for n, t in cls._fields_[-6:])
